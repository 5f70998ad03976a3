// The U-Net handle's configuration: a tiny JSON reader, parse_config (the reference's config.json -> Cfg, refusing what the executor
// does not build) and the layer list (== paddlemix_amd/unet.py:_structure).
#include "unet_exec.h"

namespace sd {
namespace unet {

// ---------------------------------------------------------------------------------------------------------------- tiny JSON
struct JVal {
  enum Kind { NUL, BOOL, NUM, STR, ARR, OBJ } kind = NUL;
  bool b = false;
  double num = 0.0;
  std::string str;
  std::vector<JVal> arr;
  std::vector<std::pair<std::string, JVal>> obj;
  const JVal* get(const std::string& k) const {
    for (auto& kv : obj)
      if (kv.first == k) return &kv.second;
    return nullptr;
  }
};
struct JParser {
  const char* p;
  int depth = 0;   // nesting of the value being parsed: a model config nests two deep; a million '[' must not be a stack overflow
  explicit JParser(const char* s) : p(s) {}
  void ws() {
    while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') ++p;
  }
  JVal parse() {
    struct Depth {
      int& d;
      explicit Depth(int& d_) : d(d_) {
        if (++d > 32) die(MI355X_SD_ERR_INVALID, "config_json: nested more than 32 levels deep");
      }
      ~Depth() { --d; }
    } guard(depth);
    ws();
    JVal v;
    if (*p == '{') {
      v.kind = JVal::OBJ;
      ++p;
      ws();
      if (*p == '}') { ++p; return v; }
      for (;;) {
        ws();
        JVal k = parse();
        if (k.kind != JVal::STR) die(MI355X_SD_ERR_INVALID, "config_json: object key is not a string");
        ws();
        if (*p != ':') die(MI355X_SD_ERR_INVALID, "config_json: expected ':'");
        ++p;
        v.obj.emplace_back(k.str, parse());
        ws();
        if (*p == ',') { ++p; continue; }
        if (*p == '}') { ++p; return v; }
        die(MI355X_SD_ERR_INVALID, "config_json: expected ',' or '}'");
      }
    }
    if (*p == '[') {
      v.kind = JVal::ARR;
      ++p;
      ws();
      if (*p == ']') { ++p; return v; }
      for (;;) {
        v.arr.push_back(parse());
        ws();
        if (*p == ',') { ++p; continue; }
        if (*p == ']') { ++p; return v; }
        die(MI355X_SD_ERR_INVALID, "config_json: expected ',' or ']'");
      }
    }
    if (*p == '"') {
      v.kind = JVal::STR;
      ++p;
      while (*p && *p != '"') {
        if (*p == '\\' && p[1]) ++p;
        v.str.push_back(*p++);
      }
      if (*p != '"') die(MI355X_SD_ERR_INVALID, "config_json: unterminated string");
      ++p;
      return v;
    }
    if (!strncmp(p, "true", 4)) { p += 4; v.kind = JVal::BOOL; v.b = true; return v; }
    if (!strncmp(p, "false", 5)) { p += 5; v.kind = JVal::BOOL; v.b = false; return v; }
    if (!strncmp(p, "null", 4)) { p += 4; return v; }
    char* end = nullptr;
    v.num = strtod(p, &end);
    if (end == p) die(MI355X_SD_ERR_INVALID, "config_json: unexpected character");
    p = end;
    v.kind = JVal::NUM;
    return v;
  }
};

// A config number that has to be an integer inside [lo, hi]: the text comes from a host (a file someone edited), and a width of
// 2^31 or a depth of 10^30 must be a refusal here -- not an out-of-range float-to-int conversion, and not a parameter table that
// exhausts the machine's memory before anything else can object (tests/test_boundary_fuzz.py).
int as_int(double x, const char* key, int lo, int hi) {
  if (!(x >= (double)lo && x <= (double)hi) || x != floor(x))
    die(MI355X_SD_ERR_INVALID, std::string("config ") + key + ": expected an integer between " + std::to_string(lo) + " and " + std::to_string(hi));
  return (int)x;
}

std::vector<int> int_or_list(const JVal* v, size_t n, int dflt, const char* key, int lo, int hi) {
  std::vector<int> out(n, dflt);
  if (!v || v->kind == JVal::NUL) return out;
  if (v->kind == JVal::NUM) return std::vector<int>(n, as_int(v->num, key, lo, hi));
  if (v->kind != JVal::ARR || v->arr.size() != n) die(MI355X_SD_ERR_INVALID, std::string("config ") + key + ": expected an int or one int per block");
  for (size_t i = 0; i < n; ++i) {
    if (v->arr[i].kind != JVal::NUM) die(MI355X_SD_ERR_UNSUPPORTED, std::string("config ") + key + ": nested lists are not implemented");
    out[i] = as_int(v->arr[i].num, key, lo, hi);
  }
  return out;
}

Cfg parse_config(const char* json) {
  JParser jp(json);
  const JVal root = jp.parse();
  if (root.kind != JVal::OBJ) die(MI355X_SD_ERR_INVALID, "config_json: expected an object");
  Cfg c;
  auto num = [&](const char* k, double d) {
    const JVal* v = root.get(k);
    return (v && v->kind == JVal::NUM) ? v->num : d;
  };
  auto boolean = [&](const char* k, bool d) {
    const JVal* v = root.get(k);
    return (v && v->kind == JVal::BOOL) ? v->b : d;
  };
  auto strs = [&](const char* k, std::vector<std::string> d) {
    const JVal* v = root.get(k);
    if (!v || v->kind != JVal::ARR) return d;
    std::vector<std::string> o;
    for (auto& e : v->arr) o.push_back(e.str);
    return o;
  };
  // what this executor does not build must not load silently (same refusals as paddlemix_amd/unet.py normalize_config)
  static const char* must_be_null[] = {
                                       "time_embedding_dim", "time_embedding_act_fn", "timestep_post_act", "cross_attention_norm",
                                       "mid_block_only_cross_attention", "reverse_transformer_layers_per_block", "num_attention_heads"};
  for (const char* k : must_be_null) {
    const JVal* v = root.get(k);
    if (v && !(v->kind == JVal::NUL || (v->kind == JVal::BOOL && !v->b)))
      die(MI355X_SD_ERR_UNSUPPORTED, std::string("mi355x_sd_unet_create: config ") + k + " is not implemented by the C executor");
  }
  static const char* must_be_false[] = {"center_input_sample", "dual_cross_attention", "only_cross_attention", "resnet_skip_time_act"};
  for (const char* k : must_be_false)
    if (boolean(k, false)) die(MI355X_SD_ERR_UNSUPPORTED, std::string("mi355x_sd_unet_create: config ") + k + "=true is not implemented");
  auto str_is = [&](const char* k, const char* want) {
    const JVal* v = root.get(k);
    if (v && v->kind == JVal::STR && v->str != want)
      die(MI355X_SD_ERR_UNSUPPORTED, std::string("mi355x_sd_unet_create: config ") + k + "=" + v->str + " is not implemented");
  };
  str_is("act_fn", "silu");
  str_is("time_embedding_type", "positional");
  str_is("resnet_time_scale_shift", "default");
  str_is("attention_type", "default");
  str_is("mid_block_type", "UNetMidBlock2DCrossAttn");
  str_is("data_format", "NCHW");
  if (const JVal* v = root.get("mid_block_type"))   // null = "no mid block" in the reference (unet_2d_condition.py:553-555)
    if (v->kind == JVal::NUL) die(MI355X_SD_ERR_UNSUPPORTED, "mi355x_sd_unet_create: config mid_block_type=null (no mid block) is not implemented");
  if (boolean("upcast_attention", false)) die(MI355X_SD_ERR_UNSUPPORTED, "mi355x_sd_unet_create: config upcast_attention=true is not implemented");
  if (num("downsample_padding", 1) != 1 || num("conv_in_kernel", 3) != 3 || num("conv_out_kernel", 3) != 3 ||
      num("resnet_out_scale_factor", 1.0) != 1.0 || num("dropout", 0.0) != 0.0)
    die(MI355X_SD_ERR_UNSUPPORTED, "mi355x_sd_unet_create: downsample_padding / conv kernels / resnet_out_scale_factor / dropout off default");

  c.in_channels = as_int(num("in_channels", 4), "in_channels", 1, 64);
  c.out_channels = as_int(num("out_channels", 4), "out_channels", 1, 64);
  c.flip_sin_to_cos = boolean("flip_sin_to_cos", true);
  c.freq_shift = num("freq_shift", 0);
  c.down = strs("down_block_types", c.down);
  c.up = strs("up_block_types", c.up);
  if (const JVal* v = root.get("block_out_channels")) {
    if (v->kind != JVal::ARR) die(MI355X_SD_ERR_INVALID, "config block_out_channels: expected a list");
    c.boc.clear();
    for (auto& e : v->arr) {
      if (e.kind != JVal::NUM) die(MI355X_SD_ERR_INVALID, "config block_out_channels: expected integers");
      if (c.boc.size() >= 8) die(MI355X_SD_ERR_INVALID, "config block_out_channels: at most 8 levels");
      c.boc.push_back(as_int(e.num, "block_out_channels", 8, 16384));
    }
  }
  const size_t n = c.down.size();
  if (c.boc.size() != n || c.up.size() != n || n < 1) die(MI355X_SD_ERR_INVALID, "config: block lists must have one entry per level");
  for (auto& bt : c.down)
    if (bt != "CrossAttnDownBlock2D" && bt != "DownBlock2D") die(MI355X_SD_ERR_UNSUPPORTED, "block type " + bt + " is not implemented");
  for (auto& bt : c.up)
    if (bt != "CrossAttnUpBlock2D" && bt != "UpBlock2D") die(MI355X_SD_ERR_UNSUPPORTED, "block type " + bt + " is not implemented");
  c.layers_per_block = int_or_list(root.get("layers_per_block"), n, 2, "layers_per_block", 1, 16);
  c.tlayers = int_or_list(root.get("transformer_layers_per_block"), n, 1, "transformer_layers_per_block", 1, 64);
  c.heads = int_or_list(root.get("attention_head_dim"), n, 8, "attention_head_dim", 1, 2048);   // the naming quirk at unet_2d_condition.py:245
  std::vector<int> cross = int_or_list(root.get("cross_attention_dim"), n, 1280, "cross_attention_dim", 8, 65536);
  for (int x : cross)
    if (x != cross[0]) die(MI355X_SD_ERR_UNSUPPORTED, "per-block cross_attention_dim is not implemented");
  c.cross_dim = cross[0];
  c.mid_scale = num("mid_block_scale_factor", 1.0);
  c.groups = as_int(num("norm_num_groups", 32), "norm_num_groups", 1, 1024);
  c.norm_eps = num("norm_eps", 1e-5);
  c.linear_proj = boolean("use_linear_projection", false);
  if (const JVal* v = root.get("addition_embed_type")) {
    if (v->kind == JVal::STR) {
      if (v->str != "text_time") die(MI355X_SD_ERR_UNSUPPORTED, "addition_embed_type=" + v->str + " is not implemented");
      c.text_time = true;
      c.atd = as_int(num("addition_time_embed_dim", 0), "addition_time_embed_dim", 0, 8192);
      c.pdim = as_int(num("projection_class_embeddings_input_dim", 0), "projection_class_embeddings_input_dim", 0, 1 << 20);
      if (c.atd <= 0 || c.pdim <= 0) die(MI355X_SD_ERR_INVALID, "text_time needs addition_time_embed_dim and projection_class_embeddings_input_dim");
    }
  }
  // projection_class_embeddings_input_dim also sizes the "projection" / "simple_projection" class embeddings
  if (const JVal* v = root.get("projection_class_embeddings_input_dim"))
    if (v->kind == JVal::NUM) c.pdim = as_int(v->num, "projection_class_embeddings_input_dim", 1, 1 << 20);
  if (const JVal* v = root.get("time_cond_proj_dim"))
    if (v->kind != JVal::NUL) {
      if (v->kind != JVal::NUM) die(MI355X_SD_ERR_INVALID, "config time_cond_proj_dim: expected an integer or null");
      c.tcp = as_int(v->num, "time_cond_proj_dim", 8, 1 << 16);
      if (c.tcp & 7) die(MI355X_SD_ERR_UNSUPPORTED, "time_cond_proj_dim must be a multiple of 8");
    }
  {
    const JVal* ct = root.get("class_embed_type");
    const JVal* nc = root.get("num_class_embeds");
    const bool has_nc = nc && nc->kind != JVal::NUL;
    if (ct && ct->kind != JVal::NUL) {
      if (ct->kind != JVal::STR) die(MI355X_SD_ERR_INVALID, "config class_embed_type: expected a string or null");
      if (ct->str == "timestep") c.class_kind = Cfg::CLASS_TIMESTEP;
      else if (ct->str == "identity") c.class_kind = Cfg::CLASS_IDENTITY;
      else if (ct->str == "projection") c.class_kind = Cfg::CLASS_PROJECTION;
      else if (ct->str == "simple_projection") c.class_kind = Cfg::CLASS_SIMPLE;
      else die(MI355X_SD_ERR_INVALID, "class_embed_type '" + ct->str + "'");   // the reference's ValueError (unet_2d_condition.py:439-441)
      if ((c.class_kind == Cfg::CLASS_PROJECTION || c.class_kind == Cfg::CLASS_SIMPLE) && c.pdim <= 0)
        die(MI355X_SD_ERR_INVALID, "`class_embed_type`: '" + ct->str + "' requires `projection_class_embeddings_input_dim` be set");
      if ((c.class_kind == Cfg::CLASS_PROJECTION || c.class_kind == Cfg::CLASS_SIMPLE) && (c.pdim & 7))
        die(MI355X_SD_ERR_UNSUPPORTED, "projection_class_embeddings_input_dim must be a multiple of 8");
    } else if (has_nc) {
      if (nc->kind != JVal::NUM) die(MI355X_SD_ERR_INVALID, "config num_class_embeds: expected an integer or null");
      c.class_kind = Cfg::CLASS_TABLE;
      c.num_class = as_int(nc->num, "num_class_embeds", 1, 1 << 24);
    }
    c.concat = boolean("class_embeddings_concat", false);
    if (c.concat && c.class_kind == Cfg::CLASS_NONE)   // the reference builds 2x-wide time_emb_proj and then feeds them the 1x embedding
      die(MI355X_SD_ERR_INVALID, "class_embeddings_concat=true needs a class embedding (class_embed_type / num_class_embeds)");
    if (c.concat && c.text_time) die(MI355X_SD_ERR_UNSUPPORTED, "class_embeddings_concat together with addition_embed_type is not implemented");
  }
  {
    const JVal* ty = root.get("encoder_hid_dim_type");
    const JVal* hd = root.get("encoder_hid_dim");
    const bool has_hd = hd && hd->kind != JVal::NUL;
    if (ty && ty->kind != JVal::NUL) {
      if (ty->kind != JVal::STR || ty->str != "ip_image_proj")   // text_proj / text_image_proj / image_proj (unet_2d_condition.py:300-335) are not built
        die(MI355X_SD_ERR_UNSUPPORTED, "mi355x_sd_unet_create: config encoder_hid_dim_type=" + (ty->kind == JVal::STR ? ty->str : std::string("?")) +
                                           " is not implemented");
      if (!has_hd) die(MI355X_SD_ERR_INVALID, "`encoder_hid_dim` has to be defined when `encoder_hid_dim_type` is set to ip_image_proj.");
      if (hd->kind != JVal::NUM) die(MI355X_SD_ERR_INVALID, "config encoder_hid_dim: expected an integer");
      c.ip = true;
      c.ehd = as_int(hd->num, "encoder_hid_dim", 8, 1 << 16);
      if (c.ehd & 7) die(MI355X_SD_ERR_UNSUPPORTED, "encoder_hid_dim must be a multiple of 8");
      c.ip_tokens = as_int(num("ip_adapter_num_tokens", 4), "ip_adapter_num_tokens", 1, 4096);
    } else if (has_hd) {
      die(MI355X_SD_ERR_UNSUPPORTED, "mi355x_sd_unet_create: config encoder_hid_dim without a type (text_proj) is not implemented");
    }
  }
  if (c.out_channels > 4) die(MI355X_SD_ERR_UNSUPPORTED, "out_channels > 4");
  if (c.in_channels <= 0 || c.out_channels <= 0 || c.cross_dim <= 0 || (c.cross_dim & 7))
    die(MI355X_SD_ERR_INVALID, "config: in_channels / out_channels / cross_attention_dim must be positive (cross_attention_dim a multiple of 8)");
  if (c.groups <= 0) die(MI355X_SD_ERR_INVALID, "config norm_num_groups must be positive");
  for (size_t i = 0; i < n; ++i) {
    // GroupNorm groups of whole channels, 16-byte channel chunks in every kernel, and heads that divide the width
    if (c.boc[i] <= 0 || c.boc[i] % c.groups || (c.boc[i] & 7))
      die(MI355X_SD_ERR_INVALID, "config block_out_channels: every entry must be a positive multiple of norm_num_groups and of 8");
    if (c.layers_per_block[i] <= 0 || c.tlayers[i] <= 0) die(MI355X_SD_ERR_INVALID, "config layers_per_block / transformer_layers_per_block must be positive");
    if (c.heads[i] <= 0 || c.boc[i] % c.heads[i] || ((c.boc[i] / c.heads[i]) & 7) || c.boc[i] / c.heads[i] > 160)
      die(MI355X_SD_ERR_INVALID, "config attention_head_dim: the head count must be positive and divide block_out_channels into head "
                                 "dims that are multiples of 8 and at most 160");
  }
  return c;
}

std::vector<Layer> structure(const Cfg& c) {   // == paddlemix_amd/unet.py:_structure
  std::vector<Layer> L;
  const int n = (int)c.boc.size();
  auto S = [](int v) { return std::to_string(v); };
  L.push_back({Layer::SKIP});
  int out_c = c.boc[0];
  for (int i = 0; i < n; ++i) {
    const int in_c = out_c;
    out_c = c.boc[i];
    for (int j = 0; j < c.layers_per_block[i]; ++j) {
      L.push_back({Layer::RESNET, "down_blocks." + S(i) + ".resnets." + S(j), j == 0 ? in_c : out_c, out_c, 1.0});
      if (c.down[i] == "CrossAttnDownBlock2D")
        L.push_back({Layer::ATTN, "down_blocks." + S(i) + ".attentions." + S(j), 0, out_c, 1.0, c.heads[i], c.tlayers[i]});
      L.push_back({Layer::SKIP});
    }
    if (i != n - 1) {
      L.push_back({Layer::DOWN, "down_blocks." + S(i) + ".downsamplers.0.conv", 0, out_c});
      L.push_back({Layer::SKIP});
    }
  }
  L.push_back({Layer::RESNET, "mid_block.resnets.0", c.boc[n - 1], c.boc[n - 1], c.mid_scale});
  L.push_back({Layer::ATTN, "mid_block.attentions.0", 0, c.boc[n - 1], 1.0, c.heads[n - 1], c.tlayers[n - 1]});
  L.push_back({Layer::RESNET, "mid_block.resnets.1", c.boc[n - 1], c.boc[n - 1], c.mid_scale});
  out_c = c.boc[n - 1];
  for (int i = 0; i < n; ++i) {
    const int ri = n - 1 - i;
    const int prev_out = out_c;
    out_c = c.boc[ri];
    const int in_c = c.boc[n - 1 - std::min(i + 1, n - 1)];
    const int nl = c.layers_per_block[ri] + 1;
    for (int j = 0; j < nl; ++j) {
      const int skip_c = (j == nl - 1) ? in_c : out_c;
      const int rin = (j == 0) ? prev_out : out_c;
      L.push_back({Layer::CAT, "", 0, skip_c});
      L.push_back({Layer::RESNET, "up_blocks." + S(i) + ".resnets." + S(j), rin + skip_c, out_c, 1.0});
      if (c.up[i] == "CrossAttnUpBlock2D")
        L.push_back({Layer::ATTN, "up_blocks." + S(i) + ".attentions." + S(j), 0, out_c, 1.0, c.heads[ri], c.tlayers[ri]});
    }
    if (i != n - 1) L.push_back({Layer::UP, "up_blocks." + S(i) + ".upsamplers.0.conv", 0, out_c});
  }
  return L;
}

}  // namespace unet
}  // namespace sd
