// The U-Net handle's launch plan for one input geometry: the C++ form of paddlemix_amd/unet.py's _UNetPlanner, stage for stage under the
// same stage names (same op sequence, same scratch names -> bit-identical results, tests/test_gpu_cexec.py). A change to one stage
// there has its counterpart in the stage of that name here.
#include "unet_exec.h"

namespace sd {
namespace unet {

struct Planner {
  Exec& e;
  const Cfg& c;
  const int B, H, W, L;
  const int RES;   // bytes per element of the residual stream
  const int ted;   // time_embed_dim
  // what crosses stages
  View emb_t, emb, cls_out;       // [emb | class_emb] as the blocks see it, its time-embedding half, where a concatenated class embedding goes
  Ref temb_all, enc_bias, self_bias;
  View kv_all, kvip_all;
  struct Sk { int C, h, w; };
  std::vector<Sk> skips;          // the skip layout: every skip tensor in production order, the up resnets, their concat buffers
  std::vector<const Layer*> ups;
  std::vector<View> cats;
  std::vector<int> cat_xc;
  int persist_n = 0, tmp_i = 0;
  explicit Planner(Exec& ex) : e(ex), c(ex.cfg), B(ex.B), H(ex.H), W(ex.W), L(ex.L), RES(ex.resid_f32 ? 4 : 2), ted(ex.cfg.boc[0] * 4) {}

  Ref sc(const std::string& name, size_t bytes) {   // named scratch, sized to its maximum use
    auto it = e.buf_index.find(name);
    if (it == e.buf_index.end()) {
      it = e.buf_index.emplace(name, (int)e.bufs.size()).first;
      e.bufs.push_back({name, 0, 0});
    }
    Exec::Buf& b = e.bufs[it->second];
    if (bytes > b.bytes) b.bytes = bytes;
    return Ref{it->second, 0, nullptr};
  }
  Ref persist(size_t bytes) { return sc("persist." + std::to_string(persist_n++), bytes < 16 ? 16 : bytes); }
  // the split-K scratch of this handle's GEMM-class launches, part of the handle's own arena (ABI 12). Same size as the Python
  // planner's (paddlemix_amd/program.py WORKSPACE_BYTES): the split count depends on it, and the two planners are bit-identical
  static constexpr size_t GEMM_WS_BYTES = (size_t)32 << 20;
  Ref gemm_ws() { return sc("gemm_ws", GEMM_WS_BYTES); }
  Ref wref(const std::string& key) {
    auto it = e.w.find(key);
    if (it == e.w.end()) die(MI355X_SD_ERR_INVALID, "internal: packed weight " + key + " missing");
    return Ref{-1, 0, e.dev_w + it->second.off};
  }
  const Packed& wp(const std::string& key) { return e.w.at(key); }
  static View view(Ref p, int rows, int C, int es = 2) { return View{p, rows, C, C, es}; }
  static bool is_set(const Ref& r) { return r.buf >= 0 || r.abs; }
  // One launch: f(x, stream) runs at replay time on the handle x. x.at() turns a Ref captured at plan time into an address (a default
  // Ref -- an absent bias, residual or mask -- into null). Closures capture by value, never a member of the planner: it is gone by then.
  template <class F>
  void emit(F f) {
    const Exec* x = &e;
    e.prog_sym.push_back([x, f](void* st) { return f(*x, st); });
  }

  // ---- launch forms (== PlanBuilder's) ----
  void linear(const View& a, const std::string& wkey, const View& out, bool bias = true, const View& R = View(), int flags = 0) {
    const Packed& w = wp(wkey + ".w");
    const int N = w.rows, K = w.cols;
    if (K != a.C || a.es != 2) die(MI355X_SD_ERR_INVALID, "internal: linear " + wkey + " operand mismatch");
    flags |= (out.es == 4 ? MI355X_SD_OUT_F32 : 0) | (R.es == 4 ? MI355X_SD_R_F32 : 0);
    const Ref wr = wref(wkey + ".w"), br = bias ? wref(wkey + ".b") : Ref(), gw = gemm_ws();
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_linear(x.at(a.p), a.ld, x.at(wr), x.at(out.p), out.ld, a.rows, N, K, (const float*)x.at(br), nullptr, 0, 0, x.at(R.p), R.ld,
                              1.0f, flags, x.at(gw), GEMM_WS_BYTES, st);
    });
  }
  void conv3(const View& v, int h, int w_, const std::string& wkey, const View& out, int stride = 1, int up = 0, Ref rowbias = Ref(),
             const View& R = View(), float out_scale = 1.0f) {
    const int Cout = wp(wkey + ".w").rows;
    if (v.es != 2) die(MI355X_SD_ERR_INVALID, "internal: conv operand is fp32");
    const int flags = (out.es == 4 ? MI355X_SD_OUT_F32 : 0) | (R.es == 4 ? MI355X_SD_R_F32 : 0) | (e.kb64.count(wkey) ? MI355X_SD_CONV_KB64 : 0);
    const Ref wr = wref(wkey + ".w"), br = wref(wkey + ".b"), gw = gemm_ws();
    const int ld_rb = is_set(rowbias) ? e.temb_total : 0;
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_conv3x3(x.at(v.p), v.ld, x.B, h, w_, v.C, stride, up, x.at(wr), x.at(out.p), out.ld, Cout, (const float*)x.at(br),
                               (const float*)x.at(rowbias), ld_rb, x.at(R.p), R.ld, out_scale, flags, x.at(gw), GEMM_WS_BYTES, st);
    });
  }
  View gnorm(const View& v, int hw, const std::string& nkey, float eps, bool silu, const View& raw16 = View()) {
    const int nws = mi355x_sd_groupnorm_workspace_floats(B, hw, v.C);
    const Ref ws = sc("gn_ws", (size_t)4 * nws), ss = sc("gn_ss", (size_t)4 * B * 2 * v.C);
    const View y = view(sc("gn", (size_t)2 * v.rows * v.C), v.rows, v.C);
    const Ref g = wref(nkey + ".g"), bt = wref(nkey + ".b");
    const int f32 = v.es == 4;
    if (!f32 && !is_set(raw16.p) && mi355x_sd_groupnorm_act_fits(hw, v.C, c.groups)) {   // one launch for small (batch, group) chunks (PlanBuilder.gnorm)
      emit([=](const Exec& x, void* st) {
        return mi355x_sd_groupnorm_act(x.at(v.p), x.B, hw, v.C, v.ld, x.cfg.groups, eps, (const float*)x.at(g), (const float*)x.at(bt), silu ? 1 : 0,
                                       x.at(y.p), y.ld, st);
      });
      return y;
    }
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_groupnorm_stats_ex(x.at(v.p), x.B, hw, v.C, v.ld, x.cfg.groups, eps, (const float*)x.at(g), (const float*)x.at(bt),
                                          (float*)x.at(ws), (float*)x.at(ss), f32, st);
    });
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_scale_shift_act_ex(x.at(v.p), x.B, hw, v.C, v.ld, (const float*)x.at(ss), silu ? 1 : 0, x.at(y.p), y.ld, f32, x.at(raw16.p),
                                          raw16.ld, st);
    });
    return y;
  }
  void lnorm(const View& v, const std::string& nkey, const View& out) {
    const Ref g = wref(nkey + ".g"), bt = wref(nkey + ".b");
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_layernorm_ex(x.at(v.p), v.rows, v.C, v.ld, (const float*)x.at(g), (const float*)x.at(bt), 1e-5f, x.at(out.p), out.ld,
                                    v.es == 4, st);
    });
  }
  View cast16(const View& v, const std::string& name) {   // 16-bit copy of fp32 rows (operand of the down / upsampling convs)
    if (v.es == 2) return v;
    const View y = view(sc(name, (size_t)2 * v.rows * v.C), v.rows, v.C);
    emit([=](const Exec& x, void* st) { return mi355x_sd_cast_rows((const float*)x.at(v.p), v.ld, x.at(y.p), y.ld, v.rows, v.C, st); });
    return y;
  }
  void sinusoid(Ref t, int t_count, int n, int dim, int group, Ref out, size_t out_off, int ldo) {   // Timesteps: t -> [n / group][group * dim]
    const int flip = c.flip_sin_to_cos ? 1 : 0;
    const float fs = (float)c.freq_shift;
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_timestep_embedding((const float*)x.at(t), t_count, n, dim, group, flip, fs, 1.0f, 10000.0f, (unsigned char*)x.at(out) + out_off,
                                          ldo, st);
    });
  }
  // softmax(q k^T * scale + bias) v per (batch, head), as PlanBuilder.sdpa: bias an additive key mask [B, skv] (fp32) broadcast over
  // heads and queries, or none; the entry is mi355x_sd_sdpa, _sdpa_ex with MI355X_SD_SDPA_LOG2, or _sdpa_accum (out += accum * ...)
  enum SdpaEntry { SDPA, SDPA_LOG2, SDPA_ACCUM };
  void sdpa(const View& q, const View& k, const View& v, const View& out, int heads, int sq, int skv, Ref bias, float scale, SdpaEntry entry = SDPA,
            float accum = 0.0f) {
    const int d = q.C / heads;
    const int64_t bias_bs = is_set(bias) ? skv : 0;
    emit([=](const Exec& x, void* st) {
      auto call = [&](auto fn, auto... tail) {
        return fn(x.at(q.p), x.at(k.p), x.at(v.p), (const float*)x.at(bias), x.at(out.p), x.B, heads, sq, skv, d, (int64_t)sq * q.ld, q.ld,
                  (int64_t)skv * k.ld, k.ld, (int64_t)skv * v.ld, v.ld, (int64_t)sq * out.ld, out.ld, bias_bs, 0, 0, scale, tail..., st);
      };
      return entry == SDPA_LOG2 ? call(mi355x_sd_sdpa_ex, MI355X_SD_SDPA_LOG2) : entry == SDPA_ACCUM ? call(mi355x_sd_sdpa_accum, accum) : call(mi355x_sd_sdpa);
    });
  }
  void attention(const View& q, const View& k, const View& v, const View& out, int heads, int sq, int skv, bool log2 = false, Ref bias = Ref()) {
    if (log2 && is_set(bias))
      // scale = ln 2: q already carries head_dim^-0.5 * log2(e) and the masked kernel exponentiates in base e (unet.py attention)
      sdpa(q, k, v, out, heads, sq, skv, bias, (float)log(2.0));
    else if (log2)
      sdpa(q, k, v, out, heads, sq, skv, Ref(), 1.0f, SDPA_LOG2);
    else
      sdpa(q, k, v, out, heads, sq, skv, bias, (float)pow((double)(q.C / heads), -0.5));   // == Python d ** -0.5 rounded to fp32
  }

  // ---- the stages ----
  void inputs() {   // staged input and output buffers
    e.in_sample = persist((size_t)4 * B * c.in_channels * H * W);
    e.in_t = persist(4);
    e.in_scale = persist(4);
    e.in_enc = persist((size_t)2 * B * L * c.cross_dim);
    e.out = persist((size_t)4 * B * c.out_channels * H * W);
  }
  // time embedding (unet_2d_condition.py:933-951): sinusoid, cond_proj, the time MLP, with the class embedding's two halves around the MLP
  void time_embedding() {
    const View t0 = view(persist((size_t)2 * B * c.boc[0]), B, c.boc[0]);
    sinusoid(e.in_t, 1, B, c.boc[0], 1, t0.p, 0, c.boc[0]);
    const View e1 = view(persist((size_t)2 * B * ted), B, ted);
    const int ted_b = ted * (c.concat ? 2 : 1);
    emb_t = view(persist((size_t)2 * B * ted_b), B, ted_b);
    emb = emb_t.cols(0, ted);                       // the time-embedding half (all of it without concat)
    cls_out = emb_t.cols(c.concat ? ted : 0, ted);   // where the class embedding goes when concatenated
    const View pre_cls = class_embedding(true);
    if (c.tcp) {   // t_emb += cond_proj(timestep_cond) (embeddings.py:284-285; zeros when the caller passes none)
      e.in_tcond = persist((size_t)2 * B * c.tcp);
      linear(view(e.in_tcond, B, c.tcp), "time_embedding.cond_proj", t0, false, t0);
    }
    linear(t0, "time_embedding.linear_1", e1, true, View(), MI355X_SD_SILU);
    linear(e1, "time_embedding.linear_2", emb, true, pre_cls);
    class_embedding(false);
  }
  // class embedding (unet_2d_condition.py:953-975), as class_embedding in unet.py: before the time MLP a gathered / identity embedding
  // is returned to ride in as the residual of its second GEMM; after it the computed kinds add into emb (concat: the upper columns)
  View class_embedding(bool before_mlp) {
    const Cfg::ClassKind ck = c.class_kind;
    if (before_mlp && ck == Cfg::CLASS_TABLE) {
      e.in_class = persist((size_t)4 * B);
      const View dst = c.concat ? cls_out : view(persist((size_t)2 * B * ted), B, ted);
      const Ref ids = e.in_class, tab = wref("class_embedding.table");
      const int dim = ted;
      emit([=](const Exec& x, void* st) { return mi355x_sd_embed_tokens((const int32_t*)x.at(ids), x.B, 1, x.at(tab), nullptr, dim, x.at(dst.p), dst.ld, st); });
      return c.concat ? View() : dst;
    }
    if (before_mlp && ck == Cfg::CLASS_IDENTITY) {
      e.in_class = persist((size_t)2 * B * ted);
      const View src = view(e.in_class, B, ted), dst = cls_out;
      if (!c.concat) return src;
      const int dim = ted;
      emit([=](const Exec& x, void* st) { return mi355x_sd_copy_rows(x.at(src.p), src.ld, x.at(dst.p), dst.ld, x.B, dim, st); });
    }
    if (before_mlp || !(ck == Cfg::CLASS_TIMESTEP || ck == Cfg::CLASS_PROJECTION || ck == Cfg::CLASS_SIMPLE)) return View();
    View cin;
    if (ck == Cfg::CLASS_TIMESTEP) {   // class_labels -> sinusoid (time_proj) -> TimestepEmbedding
      e.in_class = persist((size_t)4 * B);
      cin = view(persist((size_t)2 * B * c.boc[0]), B, c.boc[0]);
      sinusoid(e.in_class, B, B, c.boc[0], 1, cin.p, 0, cin.ld);
    } else {
      e.in_class = persist((size_t)2 * B * c.pdim);
      cin = view(e.in_class, B, c.pdim);
    }
    const View dst = c.concat ? cls_out : emb, res = c.concat ? View() : emb;
    if (ck == Cfg::CLASS_SIMPLE) {
      linear(cin, "class_embedding", dst, true, res);
    } else {
      const View c1 = view(persist((size_t)2 * B * ted), B, ted);
      linear(cin, "class_embedding.linear_1", c1, true, View(), MI355X_SD_SILU);
      linear(c1, "class_embedding.linear_2", dst, true, res);
    }
    return View();
  }
  void added_conditions() {   // text_time (unet_2d_condition.py:991-1010): emb += MLP([text_embeds | sinusoid(time_ids)])
    if (!c.text_time) return;
    e.text_dim = c.pdim - 6 * c.atd;
    e.n_ids = 6;
    if (e.text_dim <= 0 || (e.text_dim & 7)) die(MI355X_SD_ERR_UNSUPPORTED, "text_time: text_embeds width must be a positive multiple of 8");
    e.in_addin = persist((size_t)2 * B * c.pdim);
    e.in_tids = persist((size_t)4 * B * e.n_ids);
    const View a1 = view(persist((size_t)2 * B * ted), B, ted);
    sinusoid(e.in_tids, B * e.n_ids, B * e.n_ids, c.atd, e.n_ids, e.in_addin, (size_t)2 * e.text_dim, c.pdim);
    linear(view(e.in_addin, B, c.pdim), "add_embedding.linear_1", a1, true, View(), MI355X_SD_SILU);
    linear(a1, "add_embedding.linear_2", emb, true, emb);
  }
  void block_embeddings() {   // SiLU(emb) -> every resnet's time_emb_proj in one GEMM
    const View semb = view(persist((size_t)2 * B * emb_t.C), B, emb_t.C), src = emb_t;
    const int64_t n = (int64_t)B * emb_t.C;
    emit([=](const Exec& x, void* st) { return mi355x_sd_silu(x.at(src.p), x.at(semb.p), n, 0, 0, st); });
    temb_all = persist((size_t)4 * B * e.temb_total);
    linear(semb, "temb_all", view(temb_all, B, e.temb_total, 4));
  }
  // every block's cross-attention K/V of encoder_hidden_states in one GEMM; IP-Adapter (unet_2d_condition.py:1054-1061): image_embeds ->
  // ImageProjection (Linear, view [B*T, Dx], LayerNorm) -> the image tokens' K/V for every cross-attention in one GEMM
  void context_kv() {
    const int dx = c.cross_dim, T = c.ip_tokens;
    kv_all = view(persist((size_t)2 * B * L * e.kv_total), B * L, e.kv_total);
    linear(view(e.in_enc, B * L, dx), "kv_all", kv_all, false);
    if (!c.ip) return;
    e.in_image = persist((size_t)2 * B * c.ehd);
    const View raw = view(persist((size_t)2 * B * T * dx), B, T * dx);
    const View tok = view(persist((size_t)2 * B * T * dx), B * T, dx);
    linear(view(e.in_image, B, c.ehd), "encoder_hid_proj.image_embeds", raw);
    lnorm(view(raw.p, B * T, dx), "encoder_hid_proj.norm", tok);
    kvip_all = view(persist((size_t)2 * B * T * e.kv_total), B * T, e.kv_total);
    linear(tok, "kvip_all", kvip_all, false);
  }
  // the optional masks of this plan (mi355x_sd_unet_plan_ex): the handle turns them into additive biases on the device. The Python
  // planner has no such stage -- its host stages the biases themselves, in `inputs`
  void input_masks() {
    auto mask = [&](Ref& m, int64_t n) {
      m = persist((size_t)4 * n);
      const Ref src = m, bz = persist((size_t)4 * n);
      emit([=](const Exec& x, void* st) { return mi355x_sd_mask_to_bias((const float*)x.at(src), (float*)x.at(bz), n, st); });
      return bz;
    };
    if (e.plan_flags & MI355X_SD_UNET_ENC_MASK) e.enc_bias = enc_bias = mask(e.enc_mask, (int64_t)B * L);
    if (e.plan_flags & MI355X_SD_UNET_SELF_MASK) e.self_bias = self_bias = mask(e.self_mask, (int64_t)B * H * W);
  }
  void skip_layout() {   // the pre-walk: every skip connection is produced inside the buffer its up-block consumer reads
    int h = H, w_ = W, c_cur = c.boc[0];
    for (auto& d : e.layers) {
      if (d.kind == Layer::RESNET) c_cur = d.cout;
      else if (d.kind == Layer::DOWN) { h = (h + 2 - 3) / 2 + 1; w_ = (w_ + 2 - 3) / 2 + 1; }
      else if (d.kind == Layer::SKIP) skips.push_back({c_cur, h, w_});
      else if (d.kind == Layer::CAT) break;
    }
    for (auto& d : e.layers)
      if (d.kind == Layer::RESNET && d.name.rfind("up_blocks.", 0) == 0) ups.push_back(&d);
    if (ups.size() != skips.size()) die(MI355X_SD_ERR_INVALID, "internal: skip / up-resnet count mismatch");
    for (size_t u = 0; u < ups.size(); ++u) {   // up resnet u consumes skip n-1-u
      const Sk& s = skips[skips.size() - 1 - u];
      const int cx = ups[u]->cin - s.C;
      cats.push_back(view(persist((size_t)RES * B * s.h * s.w * (cx + s.C)), B * s.h * s.w, cx + s.C, RES));
      cat_xc.push_back(cx);
    }
  }
  View skip_slot(int k) const {   // where skip k is produced
    const size_t u = skips.size() - 1 - k;
    return cats[u].cols(cat_xc[u], cats[u].C - cat_xc[u]);
  }
  View x_slot(int u) const { return cats[u].cols(0, cat_xc[u]); }
  View tmp(int rows, int ch) {
    tmp_i ^= 1;
    return view(sc(std::string("x") + std::to_string(tmp_i), (size_t)RES * rows * ch), rows, ch, RES);
  }

  void resnet(const Layer& d, const View& x, int h, int w_, const View& out) {
    const int hw = h * w_, rows = B * hw, cout = d.cout;
    const bool need_short = x.C != cout;
    View x16;
    if (need_short && x.es == 4) x16 = view(sc("x16", (size_t)2 * rows * x.C), rows, x.C);
    const View g1 = gnorm(x, hw, d.name + ".norm1", (float)c.norm_eps, true, x16);
    const View h1 = view(sc("h1", (size_t)RES * rows * cout), rows, cout, RES);   // fp32 mode: GroupNorm 2 reads the unrounded conv1 output
    Ref rb = temb_all;
    rb.off += (size_t)4 * e.temb_off[d.name];
    conv3(g1, h, w_, d.name + ".conv1", h1, 1, 0, rb);
    const View g2 = gnorm(h1, hw, d.name + ".norm2", (float)c.norm_eps, true);
    View shortv = x;
    if (need_short) {
      shortv = view(sc("short", (size_t)RES * rows * cout), rows, cout, RES);
      linear(is_set(x16.p) ? x16 : x, d.name + ".conv_shortcut", shortv);
    }
    conv3(g2, h, w_, d.name + ".conv2", out, 1, 0, Ref(), shortv, (float)(1.0 / d.scale));
  }
  void transformer(const Layer& d, const View& x, int h, int w_, const View& out) {
    const int hw = h * w_, rows = B * hw, ch = x.C;
    const View g = gnorm(x, hw, d.name + ".norm", 1e-6f, false);
    const View hid = view(sc("t_h", (size_t)RES * rows * ch), rows, ch, RES);
    const View hid16 = RES == 4 ? view(sc("t_h16", (size_t)2 * rows * ch), rows, ch) : hid;   // proj_out's operand: the last FF2 writes it
    linear(g, d.name + ".proj_in", hid);
    const View ln = view(sc("t_ln", (size_t)2 * rows * ch), rows, ch);
    const View qkv = view(sc("t_qkv", (size_t)2 * rows * 3 * ch), rows, 3 * ch);
    const View ao = view(sc("t_ao", (size_t)2 * rows * ch), rows, ch);
    const View ff = view(sc("t_ff", (size_t)2 * rows * 4 * ch), rows, 4 * ch);
    for (int l = 0; l < d.layers; ++l) {
      const std::string b = d.name + ".transformer_blocks." + std::to_string(l);
      const View q2 = view(qkv.p, rows, ch);
      lnorm(hid, b + ".norm1", ln);
      linear(ln, b + ".attn1.qkv", qkv, false);
      if (is_set(self_bias) && hw != H * W)
        // the reference pads a mask of the wrong length and then fails on the shapes of the add (attention_processor.py:616-622)
        die(MI355X_SD_ERR_INVALID, "attention_mask has " + std::to_string(H * W) + " key tokens but " + b + ".attn1 attends over " +
                                       std::to_string(hw) + " latent tokens (the mask must match the token count of every attention level)");
      attention(qkv.cols(0, ch), qkv.cols(ch, ch), qkv.cols(2 * ch, ch), ao, d.heads, hw, hw, e.log2_blocks.count(b) != 0, self_bias);
      linear(ao, b + ".attn1.out", hid, true, hid);
      lnorm(hid, b + ".norm2", ln);
      linear(ln, b + ".attn2.q", q2, false);
      const int ko = e.kv_off[b];
      attention(q2, kv_all.cols(ko, ch), kv_all.cols(ko + ch, ch), ao, d.heads, hw, L, false, enc_bias);
      if (c.ip && e.ip_scale != 0.0f)   // out += scale * attention over the image tokens (IPAdapterAttnProcessor.__call__, attention_processor.py:1880-1900)
        sdpa(q2, kvip_all.cols(ko, ch), kvip_all.cols(ko + ch, ch), ao, d.heads, hw, c.ip_tokens, Ref(), (float)pow((double)(ch / d.heads), -0.5),
             SDPA_ACCUM, e.ip_scale);
      linear(ao, b + ".attn2.out", hid, true, hid);
      lnorm(hid, b + ".norm3", ln);
      linear(ln, b + ".ff1", ff, true, View(), MI355X_SD_GEGLU);
      linear(ff, b + ".ff2", l == d.layers - 1 ? hid16 : hid, true, hid);
    }
    linear(hid16, d.name + ".proj_out", out, true, x);
  }
  void downsample(const Layer& d, const View& x, int h, int w_, const View& out) { conv3(cast16(x, "xc16"), h, w_, d.name, out, 2); }
  void upsample(const Layer& d, const View& x, int h, int w_, int ht, int wt, const View& out) {   // to the size of the skip the next resnet reads
    const View src = cast16(x, "xc16");
    if (ht == 2 * h && wt == 2 * w_) return conv3(src, h, w_, d.name, out, 1, 1);   // nearest x2 folded into the conv's gather
    // `forward_upsample_size`: a skip of odd size 2h - 1. The cropped nearest-x2 tensor is materialised (strided row copies, one per
    // source row and parity) and a plain 3x3 conv follows -- the same launches, for the same reason, as upsample in paddlemix_amd/unet.py
    if (!((ht == 2 * h - 1 || ht == 2 * h) && (wt == 2 * w_ - 1 || wt == 2 * w_))) die(MI355X_SD_ERR_INVALID, "internal: upsample target size");
    const int C_ = src.C, lds = src.ld;
    const View upb = view(sc("upx", (size_t)2 * B * ht * wt * C_), B * ht * wt, C_);
    for (int b = 0; b < B; ++b)
      for (int i_ = 0; i_ < h; ++i_)
        for (int dy = 0; dy < 2; ++dy) {
          const int y = 2 * i_ + dy;
          if (y >= ht) continue;
          for (int dx = 0; dx < 2; ++dx) {
            const int n = (wt - dx + 1) / 2;
            Ref sp = src.p, dp = upb.p;
            sp.off += (size_t)2 * ((size_t)(b * h + i_) * w_) * src.ld;
            dp.off += (size_t)2 * ((size_t)(b * ht + y) * wt + dx) * C_;
            emit([=](const Exec& x_, void* st) { return mi355x_sd_copy_rows(x_.at(sp), lds, x_.at(dp), 2 * C_, n, C_, st); });
          }
        }
    conv3(upb, ht, wt, d.name, out);
  }
  // every skip tensor and the mid output are complete and consumed here: record their shapes (mi355x_sd_unet_skip_shape) and, with
  // ControlNet residuals planned, add them in place (unet_2d_condition.py:1121-1132, 1151-1155)
  void controlnet_residuals(const View& mid, int h, int w_) {
    e.skip_shapes.clear();
    for (auto& sk : skips) e.skip_shapes.push_back({sk.C, sk.h, sk.w});
    e.skip_shapes.push_back({mid.C, h, w_});
    if (!(e.plan_flags & MI355X_SD_UNET_CONTROLNET)) return;
    const int f32 = RES == 4 ? 1 : 0;
    auto add = [&](const View& dst, int C, int64_t hw) {
      const Ref r = persist((size_t)4 * B * C * hw);
      emit([=](const Exec& x, void* st) { return mi355x_sd_add_nchw_ex(x.at(dst.p), dst.ld, (const float*)x.at(r), x.B, C, hw, f32, st); });
      return r;
    };
    e.ctrl_down.clear();
    for (size_t k = 0; k < skips.size(); ++k) e.ctrl_down.push_back(add(skip_slot((int)k), skips[k].C, (int64_t)skips[k].h * skips[k].w));
    e.ctrl_mid = add(mid, mid.C, (int64_t)h * w_);
  }
  // FreeU (apply_freeu, unet_2d_blocks.py:2329-2351, 2478-2500): the concat input of up resnet u, in place, before its first GroupNorm --
  // backbone half * b, skip planes Fourier-filtered with scale s, for the resnets of up blocks 0 (b1, s1) and 1 (b2, s2)
  void freeu(int u) {
    if (!e.freeu) return;
    const std::string& name = ups[u]->name;
    const int i = name.rfind("up_blocks.0.", 0) == 0 ? 0 : name.rfind("up_blocks.1.", 0) == 0 ? 1 : -1;
    if (i < 0) return;
    const View cat = cats[u];
    const Sk& s = skips[skips.size() - 1 - u];
    const int h = s.h, w_ = s.w, cx = cat_xc[u], cs = cat.C - cat_xc[u], f32 = cat.es == 4;
    const float b = e.freeu_b[i], sc_ = e.freeu_s[i];
    const Ref ws = sc("freeu_ws", (size_t)4 * mi355x_sd_freeu_workspace_floats(B, h, w_, cs));
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_freeu(x.at(cat.p), cat.ld, x.B, h, w_, cx, cs, b, sc_, f32, (float*)x.at(ws), st);
    });
  }
  View stem() {   // conv_in writes skip 0
    const View cur = skip_slot(0);
    const Ref smp = e.in_sample, scl = e.in_scale, wr = wref("conv_in.w"), br = wref("conv_in.b");
    const int ci = c.in_channels, Hc = H, Wc = W, co = c.boc[0];
    emit([=](const Exec& x, void* st) {
      return mi355x_sd_conv_in3x3_ex((const float*)x.at(smp), (const float*)x.at(scl), x.at(wr), (const float*)x.at(br), x.at(cur.p), x.B, ci, Hc,
                                     Wc, co, cur.ld, cur.es == 4, st);
    });
    return cur;
  }
  View walk() {   // the loop over the layer list that picks each layer's destination; returns the last output
    int h = H, w_ = W, k = 1, u = 0;   // next skip to produce (conv_in made skip 0), next up resnet
    View cur = stem();
    const size_t nl = e.layers.size();
    for (size_t i = 1; i < nl; ++i) {
      const Layer& d = e.layers[i];
      const bool last = i + 1 >= nl;
      const Layer::Kind nxt = last ? Layer::SKIP : e.layers[i + 1].kind;
      const int rows = B * h * w_;
      if (d.kind == Layer::RESNET || d.kind == Layer::ATTN) {
        View dst;
        if (!last && nxt == Layer::SKIP) dst = skip_slot(k);
        else if (!last && nxt == Layer::CAT) dst = x_slot(u);
        else dst = tmp(rows, d.cout);   // followed by a transformer / the mid resnet / an upsampler / the head
        if (d.kind == Layer::RESNET) resnet(d, cur, h, w_, dst);
        else transformer(d, cur, h, w_, dst);
        cur = dst;
      } else if (d.kind == Layer::SKIP) {
        ++k;
      } else if (d.kind == Layer::DOWN) {
        const View dst = skip_slot(k);
        downsample(d, cur, h, w_, dst);
        h = (h + 2 - 3) / 2 + 1;
        w_ = (w_ + 2 - 3) / 2 + 1;
        cur = dst;
      } else if (d.kind == Layer::CAT) {
        if (u == 0) controlnet_residuals(cur, h, w_);
        freeu(u);
        cur = cats[u++];
      } else if (d.kind == Layer::UP) {
        const View dst = x_slot(u);
        const Sk& tgt = skips[skips.size() - 1 - u];
        upsample(d, cur, h, w_, tgt.h, tgt.w, dst);
        h = tgt.h;
        w_ = tgt.w;
        cur = dst;
      }
    }
    if (k != (int)skips.size() || u != (int)ups.size() || h != H || w_ != W) die(MI355X_SD_ERR_INVALID, "internal: plan walk mismatch");
    return cur;
  }
  void head(const View& x) {   // conv_norm_out + conv_out (unet_2d_condition.py:1193-1196)
    const View g = gnorm(x, H * W, "conv_norm_out", (float)c.norm_eps, true);
    const Ref wr = wref("conv_out.w"), br = wref("conv_out.b"), o = e.out;
    const int Hc = H, Wc = W, co = c.out_channels;
    emit([=](const Exec& x_, void* st) {
      return mi355x_sd_conv_out3x3(x_.at(g.p), g.ld, x_.at(wr), (const float*)x_.at(br), (float*)x_.at(o), x_.B, g.C, Hc, Wc, co, st);
    });
  }
  void layout() {   // place every buffer in the workspace
    size_t off = 0;
    for (auto& b : e.bufs) {
      b.off = off;
      off += (b.bytes + 255) & ~(size_t)255;
    }
    e.workspace_bytes = off;
  }
};

void build_plan(Exec& e) {
  Planner p(e);
  p.inputs();
  p.time_embedding();
  p.added_conditions();
  p.block_embeddings();
  p.context_kv();
  p.input_masks();
  p.skip_layout();
  p.head(p.walk());
  p.layout();
}

}  // namespace unet
}  // namespace sd
