// The U-Net handle's weights: the parameter table a host loads against (== unet_param_shapes) and the packer that turns the loaded
// fp32 tensors into the kernels' layouts once (== UNet2DConditionModel._load_weights, stage for stage, bit for bit).
#include "unet_exec.h"

namespace sd {
namespace unet {

// fp32 -> the build's 16-bit element, round to nearest even (what torch's .to(bfloat16 / float16) does)
uint16_t to_elem16(float f) {
#ifdef MI355X_SD_F16
  _Float16 x = (_Float16)f;
  uint16_t h;
  memcpy(&h, &x, 2);
  return h;
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
#endif
}

void expect(Exec& e, const std::string& name, std::vector<int64_t> shape) {
  e.params[name].shape = std::move(shape);
  e.order.push_back(name);
}

void build_param_table(Exec& e) {   // == unet_param_shapes for the supported configs
  const Cfg& c = e.cfg;
  const int ted = c.boc[0] * 4;
  auto lin = [&](const std::string& n, int i, int o, bool bias = true) {
    expect(e, n + ".weight", {i, o});
    if (bias) expect(e, n + ".bias", {o});
  };
  auto conv = [&](const std::string& n, int i, int o, int k) {
    expect(e, n + ".weight", {o, i, k, k});
    expect(e, n + ".bias", {o});
  };
  auto norm = [&](const std::string& n, int ch) {
    expect(e, n + ".weight", {ch});
    expect(e, n + ".bias", {ch});
  };
  conv("conv_in", c.in_channels, c.boc[0], 3);
  lin("time_embedding.linear_1", c.boc[0], ted);
  if (c.tcp) lin("time_embedding.cond_proj", c.tcp, c.boc[0], false);
  lin("time_embedding.linear_2", ted, ted);
  if (c.class_kind == Cfg::CLASS_TABLE) {
    expect(e, "class_embedding.weight", {c.num_class, ted});   // nn.Embedding [classes, dim]: a table, never transposed
  } else if (c.class_kind == Cfg::CLASS_TIMESTEP || c.class_kind == Cfg::CLASS_PROJECTION) {
    lin("class_embedding.linear_1", c.class_kind == Cfg::CLASS_TIMESTEP ? c.boc[0] : c.pdim, ted);
    lin("class_embedding.linear_2", ted, ted);
  } else if (c.class_kind == Cfg::CLASS_SIMPLE) {
    lin("class_embedding", c.pdim, ted);
  }
  if (c.text_time) {
    lin("add_embedding.linear_1", c.pdim, ted);
    lin("add_embedding.linear_2", ted, ted);
  }
  for (auto& d : e.layers) {
    if (d.kind == Layer::RESNET) {
      norm(d.name + ".norm1", d.cin);
      conv(d.name + ".conv1", d.cin, d.cout, 3);
      lin(d.name + ".time_emb_proj", ted * (c.concat ? 2 : 1), d.cout);
      norm(d.name + ".norm2", d.cout);
      conv(d.name + ".conv2", d.cout, d.cout, 3);
      if (d.cin != d.cout) conv(d.name + ".conv_shortcut", d.cin, d.cout, 1);
    } else if (d.kind == Layer::ATTN) {
      const int ch = d.cout;
      norm(d.name + ".norm", ch);
      if (c.linear_proj) lin(d.name + ".proj_in", ch, ch);
      else conv(d.name + ".proj_in", ch, ch, 1);
      for (int l = 0; l < d.layers; ++l) {
        const std::string b = d.name + ".transformer_blocks." + std::to_string(l);
        norm(b + ".norm1", ch);
        for (int a = 0; a < 2; ++a) {
          const std::string an = b + (a == 0 ? ".attn1" : ".attn2");
          const int kd = a == 0 ? ch : c.cross_dim;
          lin(an + ".to_q", ch, ch, false);
          lin(an + ".to_k", kd, ch, false);
          lin(an + ".to_v", kd, ch, false);
          lin(an + ".to_out.0", ch, ch);
          if (a == 0) {
            norm(b + ".norm2", ch);
          } else if (c.ip) {   // IPAdapterAttnProcessor (attention_processor.py:1816-1817)
            lin(an + ".processor.to_k_ip", kd, ch, false);
            lin(an + ".processor.to_v_ip", kd, ch, false);
          }
        }
        norm(b + ".norm3", ch);
        lin(b + ".ff.net.0.proj", ch, 8 * ch);
        lin(b + ".ff.net.2", 4 * ch, ch);
      }
      if (c.linear_proj) lin(d.name + ".proj_out", ch, ch);
      else conv(d.name + ".proj_out", ch, ch, 1);
    } else if (d.kind == Layer::DOWN || d.kind == Layer::UP) {
      conv(d.name, d.cout, d.cout, 3);
    }
  }
  norm("conv_norm_out", c.boc[0]);
  conv("conv_out", c.boc[0], c.out_channels, 3);
  if (c.ip) {   // ImageProjection; last, like unet_param_shapes
    lin("encoder_hid_proj.image_embeds", c.ehd, c.ip_tokens * c.cross_dim);
    norm("encoder_hid_proj.norm", c.cross_dim);
  }
}

// ---- packing (== UNet2DConditionModel._load_weights) ----
struct Packer {
  Exec& e;
  explicit Packer(Exec& ex) : e(ex) {}
  const HostT& get(const std::string& n) {
    auto it = e.params.find(n);
    if (it == e.params.end() || !it->second.loaded) die(MI355X_SD_ERR_INVALID, "missing parameter " + n);
    return it->second;
  }
  // every packed tensor is staged in its own buffer (pointers stay valid while others are added) and laid out at the end
  std::map<std::string, std::vector<unsigned char>> staged;
  std::vector<std::string> staged_order;
  unsigned char* reserve(const std::string& key, size_t bytes, int rows, int cols) {
    if (staged.count(key)) die(MI355X_SD_ERR_INVALID, "internal: packed tensor " + key + " defined twice");
    std::vector<unsigned char>& v = staged[key];
    v.resize(bytes);
    staged_order.push_back(key);
    e.w[key] = Packed{0, bytes, rows, cols};
    return v.data();
  }
  uint16_t* m16(const std::string& key, int rows, int cols) {
    return reinterpret_cast<uint16_t*>(reserve(key, (size_t)rows * cols * 2, rows, cols));
  }
  float* f32(const std::string& key, int n) { return reinterpret_cast<float*>(reserve(key, (size_t)n * 4, 1, n)); }
  // Paddle Linear [in, out] -> rows [out][in] appended at row r0 of dst (row length in); mul: fp32 factor applied before rounding
  static void lin_rows(const HostT& t, uint16_t* dst, int r0, float mul = 1.0f) {
    const int in = (int)t.shape[0], out = (int)t.shape[1];
    for (int o = 0; o < out; ++o)
      for (int i = 0; i < in; ++i) dst[(size_t)(r0 + o) * in + i] = to_elem16(mul == 1.0f ? t.v[(size_t)i * out + o] : t.v[(size_t)i * out + o] * mul);
  }
  void put_vec(const std::string& key, const std::string& name) {
    const HostT& t = get(name);
    memcpy(f32(key, (int)t.numel()), t.v.data(), t.numel() * 4);
  }
  void put_lin(const std::string& key, const std::string& name, bool bias = true) {
    const HostT& t = get(name + ".weight");
    lin_rows(t, m16(key + ".w", (int)t.shape[1], (int)t.shape[0]), 0);
    if (bias) put_vec(key + ".b", name + ".bias");
  }
  // OIHW -> [O][kh][kw][I]; 3x3 with I % 64 == 0 -> [O][I/64][kh][kw][64] (MI355X_SD_CONV_KB64: taps innermost per 64-channel block)
  void put_conv(const std::string& key, const std::string& name) {
    const HostT& t = get(name + ".weight");
    const int O = (int)t.shape[0], I = (int)t.shape[1], kh = (int)t.shape[2], kw = (int)t.shape[3];
    const bool kb64 = kh == 3 && (I % 64) == 0;
    if (kb64) e.kb64.insert(key);
    uint16_t* d = m16(key + ".w", O, kh * kw * I);
    for (int o = 0; o < O; ++o)
      for (int i = 0; i < I; ++i)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x) {
            const size_t dst = kb64 ? ((((size_t)o * (I / 64) + i / 64) * kh + y) * kw + x) * 64 + i % 64
                                    : (((size_t)o * kh + y) * kw + x) * I + i;
            d[dst] = to_elem16(t.v[(((size_t)o * I + i) * kh + y) * kw + x]);
          }
    put_vec(key + ".b", name + ".bias");
  }
  void put_norm(const std::string& key, const std::string& name) {
    put_vec(key + ".g", name + ".weight");
    put_vec(key + ".b", name + ".bias");
  }
  // ---- the stages of UNet2DConditionModel._load_weights, same names, same order of packed tensors ----
  void stem() {   // conv_in, the embeddings, and where every layer's rows sit in the batched matrices
    const Cfg& c = e.cfg;
    {   // conv_in: -> [ky][kx][ci][O]
      const HostT& t = get("conv_in.weight");
      const int O = (int)t.shape[0], I = (int)t.shape[1];
      uint16_t* d = m16("conv_in.w", 9 * I, O);
      for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i)
          for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) d[(((size_t)y * 3 + x) * I + i) * O + o] = to_elem16(t.v[(((size_t)o * I + i) * 3 + y) * 3 + x]);
      put_vec("conv_in.b", "conv_in.bias");
    }
    put_lin("time_embedding.linear_1", "time_embedding.linear_1");
    put_lin("time_embedding.linear_2", "time_embedding.linear_2");
    if (c.tcp) put_lin("time_embedding.cond_proj", "time_embedding.cond_proj", false);
    if (c.class_kind == Cfg::CLASS_TABLE) {
      const HostT& t = get("class_embedding.weight");
      uint16_t* d = m16("class_embedding.table", (int)t.shape[0], (int)t.shape[1]);
      for (size_t i = 0; i < t.numel(); ++i) d[i] = to_elem16(t.v[i]);
    } else if (c.class_kind == Cfg::CLASS_TIMESTEP || c.class_kind == Cfg::CLASS_PROJECTION) {
      put_lin("class_embedding.linear_1", "class_embedding.linear_1");
      put_lin("class_embedding.linear_2", "class_embedding.linear_2");
    } else if (c.class_kind == Cfg::CLASS_SIMPLE) {
      put_lin("class_embedding", "class_embedding");
    }
    if (c.text_time) {
      put_lin("add_embedding.linear_1", "add_embedding.linear_1");
      put_lin("add_embedding.linear_2", "add_embedding.linear_2");
    }
    int toff = 0, koff = 0;
    for (auto& d : e.layers) {
      if (d.kind == Layer::RESNET) {
        e.temb_off[d.name] = toff;
        toff += d.cout;
      } else if (d.kind == Layer::ATTN) {
        for (int l = 0; l < d.layers; ++l) {
          e.kv_off[d.name + ".transformer_blocks." + std::to_string(l)] = koff;
          koff += 2 * d.cout;
        }
      }
    }
    e.temb_total = toff;
    e.kv_total = koff;
  }
  void resnet(const Layer& d) {   // (time_emb_proj: a row block of temb_all, see batched())
    put_norm(d.name + ".norm1", d.name + ".norm1");
    put_conv(d.name + ".conv1", d.name + ".conv1");
    put_norm(d.name + ".norm2", d.name + ".norm2");
    put_conv(d.name + ".conv2", d.name + ".conv2");
    if (d.cin != d.cout) put_conv(d.name + ".conv_shortcut", d.name + ".conv_shortcut");
  }
  void transformer(const Layer& d) {
    put_norm(d.name + ".norm", d.name + ".norm");
    if (e.cfg.linear_proj) {
      put_lin(d.name + ".proj_in", d.name + ".proj_in");
      put_lin(d.name + ".proj_out", d.name + ".proj_out");
    } else {
      put_conv(d.name + ".proj_in", d.name + ".proj_in");
      put_conv(d.name + ".proj_out", d.name + ".proj_out");
    }
    for (int l = 0; l < d.layers; ++l) transformer_block(d, d.name + ".transformer_blocks." + std::to_string(l));
  }
  void transformer_block(const Layer& d, const std::string& b) {   // (attn2.to_k / to_v: a row block of kv_all, see batched())
    const int ch = d.cout;
    for (const char* nm : {".norm1", ".norm2", ".norm3"}) put_norm(b + nm, b + nm);
    uint16_t* q = m16(b + ".attn1.qkv.w", 3 * ch, ch);
    float qmul = 1.0f;
    if (e.fold_scale && ch / d.heads == 64) {
      qmul = (float)(pow((double)(ch / d.heads), -0.5) * 1.4426950408889634);
      e.log2_blocks.insert(b);
    }
    lin_rows(get(b + ".attn1.to_q.weight"), q, 0, qmul);
    lin_rows(get(b + ".attn1.to_k.weight"), q, ch);
    lin_rows(get(b + ".attn1.to_v.weight"), q, 2 * ch);
    lin_rows(get(b + ".attn2.to_q.weight"), m16(b + ".attn2.q.w", ch, ch), 0);
    put_lin(b + ".attn1.out", b + ".attn1.to_out.0");
    put_lin(b + ".attn2.out", b + ".attn2.to_out.0");
    // GEGLU: rows interleaved [16 value | 16 gate]
    const HostT& t = get(b + ".ff.net.0.proj.weight");   // [c, 8c]
    const HostT& tb = get(b + ".ff.net.0.proj.bias");
    const int in = (int)t.shape[0], out = (int)t.shape[1], half = out / 2;
    uint16_t* d1 = m16(b + ".ff1.w", out, in);
    float* b1 = f32(b + ".ff1.b", out);
    for (int o = 0; o < out; ++o) {
      const int src = o < half ? o : o - half;            // value rows come from [0, half), gate rows from [half, out)
      const int grp = src / 16, r = src % 16;
      const int dst = grp * 32 + (o < half ? 0 : 16) + r;
      for (int i = 0; i < in; ++i) d1[(size_t)dst * in + i] = to_elem16(t.v[(size_t)i * out + o]);
      b1[dst] = tb.v[o];
    }
    put_lin(b + ".ff2", b + ".ff.net.2");
  }
  void sampler(const Layer& d) { put_conv(d.name, d.name); }
  void batched() {   // what the layers contribute to the one-GEMM-per-step matrices
    const Cfg& c = e.cfg;
    {   // every cross-attention to_k / to_v in one matrix
      uint16_t* kv = m16("kv_all.w", e.kv_total, c.cross_dim);
      for (auto& d : e.layers)
        if (d.kind == Layer::ATTN)
          for (int l = 0; l < d.layers; ++l) {
            const std::string b = d.name + ".transformer_blocks." + std::to_string(l);
            const int r0 = e.kv_off[b];
            lin_rows(get(b + ".attn2.to_k.weight"), kv, r0);
            lin_rows(get(b + ".attn2.to_v.weight"), kv, r0 + d.cout);
          }
    }
    if (c.ip) {   // ... and every IPAdapterAttnProcessor's to_k_ip / to_v_ip at the same row offsets
      uint16_t* kv = m16("kvip_all.w", e.kv_total, c.cross_dim);
      for (auto& d : e.layers)
        if (d.kind == Layer::ATTN)
          for (int l = 0; l < d.layers; ++l) {
            const std::string b = d.name + ".transformer_blocks." + std::to_string(l);
            const int r0 = e.kv_off[b];
            lin_rows(get(b + ".attn2.processor.to_k_ip.weight"), kv, r0);
            lin_rows(get(b + ".attn2.processor.to_v_ip.weight"), kv, r0 + d.cout);
          }
      put_lin("encoder_hid_proj.image_embeds", "encoder_hid_proj.image_embeds");
      put_norm("encoder_hid_proj.norm", "encoder_hid_proj.norm");
    }
    {   // every resnet time_emb_proj in one matrix
      uint16_t* tw = m16("temb_all.w", e.temb_total, c.boc[0] * 4 * (c.concat ? 2 : 1));
      float* tb = f32("temb_all.b", e.temb_total);
      for (auto& d : e.layers)
        if (d.kind == Layer::RESNET) {
          const int r0 = e.temb_off[d.name];
          lin_rows(get(d.name + ".time_emb_proj.weight"), tw, r0);
          const HostT& bb = get(d.name + ".time_emb_proj.bias");
          memcpy(tb + r0, bb.v.data(), bb.numel() * 4);
        }
    }
  }
  void head() {
    put_norm("conv_norm_out", "conv_norm_out");
    put_conv("conv_out", "conv_out");
  }
  void layout() {   // place the staged tensors in the image and release the fp32 host copies
    size_t off = 0;
    for (auto& key : staged_order) {
      e.w[key].off = off;
      off += (staged[key].size() + 255) & ~(size_t)255;
    }
    e.weight_bytes = off;
    e.host_pack.assign(off, 0);
    for (auto& key : staged_order) {
      memcpy(e.host_pack.data() + e.w[key].off, staged[key].data(), staged[key].size());
      std::vector<unsigned char>().swap(staged[key]);
    }
    for (auto& kv : e.params) {   // the fp32 host copies are no longer needed
      std::vector<float>().swap(kv.second.v);
    }
  }
};

void pack_weights(Exec& e) {
  Packer p(e);
  p.stem();
  for (auto& d : e.layers) {
    if (d.kind == Layer::RESNET) p.resnet(d);
    else if (d.kind == Layer::ATTN) p.transformer(d);
    else if (d.kind == Layer::DOWN || d.kind == Layer::UP) p.sampler(d);
  }
  p.batched();
  p.head();
  p.layout();
}

}  // namespace unet
}  // namespace sd
