// Seam B1 in the C ABI: UNet2DConditionModel as an opaque handle -- config in, weights in, one call per denoising step.
//
//   mi355x_sd_unet_create(config_json, &h)            parse the reference's config.json, build the layer list
//   mi355x_sd_unet_load_weight(h, name, ptr, ...)     reference parameter names, Paddle layouts (Linear [in,out], conv OIHW), host memory
//   mi355x_sd_unet_weight_bytes / _finalize_weights   pack once (transposes, fused QKV, batched K/V and time projections, GEGLU
//                                                     interleave) into a CALLER-OWNED device buffer
//   mi355x_sd_unet_plan(h, B, H, W, L, &bytes)        static program + workspace layout for one input geometry
//   mi355x_sd_unet_bind_workspace(h, ptr, bytes)      caller-owned device arena; nothing is allocated on the device by the library
//   mi355x_sd_unet_forward(h, stream, ...)            stage inputs + replay the program (optionally as a hipGraph)
//
// It is the C++ form of paddlemix_amd/unet.py (same op sequence, same packing -> bit-identical results, tested) for the
// configurations of the hot path: the four SD block types, mid cross-attention block, conv or linear projections,
// addition_embed_type None | "text_time", 16-bit or fp32 residual stream. Reference: UNet2DConditionModel.forward
// (ppdiffusers/ppdiffusers/models/unet_2d_condition.py:809-1207); the opaque-predictor precedent for this seam is
// PaddleInferRuntimeModel.__call__ (ppdiffusers/ppdiffusers/models/paddleinfer_runtime.py:47-126) with the named inputs of
// ppdiffusers/deploy/sd15/export_model.py:78-90 (sample, timestep, encoder_hidden_states [+ text_embeds, time_ids]).
// This file holds the handle's C entry points; the config, the weights and the plan are unet_config.hip, unet_weights.hip and
// unet_plan.hip (shared types: unet_exec.h).
#include "unet_exec.h"

using namespace sd::unet;

namespace {

float bf16_bits_to_f32(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
float f16_bits_to_f32(uint16_t h) {
  _Float16 x;
  memcpy(&x, &h, 2);
  return (float)x;
}
int report(const std::exception& x) {   // the planner's own refusal with its code, or whatever else was thrown (bad_alloc ...)
  const ExecError* own = dynamic_cast<const ExecError*>(&x);
  sd::set_last_error(own ? x.what() : (std::string("mi355x_sd_unet: ") + x.what()).c_str());
  return own ? own->code : (int)MI355X_SD_ERR_INVALID;
}
Exec* H_(void* h) { return reinterpret_cast<Exec*>(h); }

}  // namespace

extern "C" {

int mi355x_sd_unet_create(const char* config_json, void** handle) {
  if (!config_json || !handle) {
    sd::set_last_error("mi355x_sd_unet_create: null pointer");
    return MI355X_SD_ERR_INVALID;
  }
  try {
    std::unique_ptr<Exec> e(new Exec);
    e->cfg = parse_config(config_json);
    e->layers = structure(e->cfg);
    build_param_table(*e);
    *handle = e.release();
    return MI355X_SD_OK;
  } catch (const std::exception& x) {   // bad_alloc, a malformed number in the config ...: never across the C boundary
    return report(x);
  }
}

int mi355x_sd_unet_destroy(void* handle) {
  if (!handle) return MI355X_SD_OK;
  Exec* e = H_(handle);
  if (e->graph) (void)hipGraphExecDestroy(e->graph);
  delete e;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_set_option(void* handle, const char* key, int value) {
  if (!handle || !key) {
    sd::set_last_error("mi355x_sd_unet_set_option: null pointer");
    return MI355X_SD_ERR_INVALID;
  }
  Exec* e = H_(handle);
  if (!strcmp(key, "residual_f32")) {
    if (e->planned) {
      sd::set_last_error("mi355x_sd_unet_set_option: residual_f32 must be set before mi355x_sd_unet_plan");
      return MI355X_SD_ERR_INVALID;
    }
    e->resid_f32 = value != 0;
    return MI355X_SD_OK;
  }
  if (!strcmp(key, "fold_softmax_scale")) {
    if (e->packed || e->dev_w) {
      sd::set_last_error("mi355x_sd_unet_set_option: fold_softmax_scale must be set before the weights are packed");
      return MI355X_SD_ERR_INVALID;
    }
    e->fold_scale = value != 0;
    return MI355X_SD_OK;
  }
  sd::set_last_error("mi355x_sd_unet_set_option: unknown option");
  return MI355X_SD_ERR_INVALID;
}

int mi355x_sd_unet_set_ip_adapter_scale(void* handle, float scale) {
  Exec* e = H_(handle);
  if (!handle || !e->cfg.ip) {
    sd::set_last_error("mi355x_sd_unet_set_ip_adapter_scale: this UNet has no IP-Adapter (config encoder_hid_dim_type != 'ip_image_proj')");
    return MI355X_SD_ERR_INVALID;
  }
  if (!(scale == scale) || scale - scale != 0.0f) {
    sd::set_last_error("mi355x_sd_unet_set_ip_adapter_scale: scale must be finite");
    return MI355X_SD_ERR_INVALID;
  }
  if (scale != e->ip_scale && e->planned) {   // the scale is a constant of the planned launches: the plan (and its graph) go
    e->drop_graph();
    e->drop_plan();
  }
  e->ip_scale = scale;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_set_freeu(void* handle, int enabled, float s1, float s2, float b1, float b2) {
  if (!handle) {
    sd::set_last_error("mi355x_sd_unet_set_freeu: null handle");
    return MI355X_SD_ERR_INVALID;
  }
  Exec* e = H_(handle);
  for (float v : {s1, s2, b1, b2})
    if (v - v != 0.0f) {
      sd::set_last_error("mi355x_sd_unet_set_freeu: s1, s2, b1, b2 must be finite");
      return MI355X_SD_ERR_INVALID;
    }
  const bool on = enabled != 0;
  const bool same = on == e->freeu && (!on || (s1 == e->freeu_s[0] && s2 == e->freeu_s[1] && b1 == e->freeu_b[0] && b2 == e->freeu_b[1]));
  if (!same && e->planned) {   // constants of the planned launches: the plan (and its graph) go
    e->drop_graph();
    e->drop_plan();
  }
  e->freeu = on;
  if (on) {
    e->freeu_s[0] = s1; e->freeu_s[1] = s2;
    e->freeu_b[0] = b1; e->freeu_b[1] = b2;
  }
  return MI355X_SD_OK;
}

int mi355x_sd_unet_num_params(void* handle) { return handle ? (int)H_(handle)->order.size() : -1; }

int mi355x_sd_unet_param_info(void* handle, int index, const char** name, int64_t* shape4, int* ndim) {
  if (!handle || index < 0 || index >= (int)H_(handle)->order.size() || !name || !shape4 || !ndim) {
    sd::set_last_error("mi355x_sd_unet_param_info: bad argument");
    return MI355X_SD_ERR_INVALID;
  }
  Exec* e = H_(handle);
  const std::string& n = e->order[index];
  const HostT& t = e->params[n];
  *name = n.c_str();
  *ndim = (int)t.shape.size();
  for (int i = 0; i < 4; ++i) shape4[i] = i < *ndim ? t.shape[i] : 1;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_load_weight(void* handle, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
  if (!handle || !name || !host_ptr || !shape) {
    sd::set_last_error("mi355x_sd_unet_load_weight: null pointer");
    return MI355X_SD_ERR_INVALID;
  }
  try {
    Exec* e = H_(handle);
    if (e->dev_w || e->packed) die(MI355X_SD_ERR_INVALID, "mi355x_sd_unet_load_weight: weights are already packed / finalized");
    auto it = e->params.find(name);
    if (it == e->params.end()) die(MI355X_SD_ERR_INVALID, std::string("mi355x_sd_unet_load_weight: the configured UNet has no parameter ") + name);
    HostT& t = it->second;
    bool same = (int)t.shape.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = t.shape[i] == shape[i];
    if (!same) die(MI355X_SD_ERR_INVALID, std::string("mi355x_sd_unet_load_weight: ") + name + ": shape differs from the configured model (Paddle layouts expected)");
    const int64_t n = t.numel();
    t.v.resize(n);
    if (dtype == MI355X_SD_DTYPE_F32) {
      memcpy(t.v.data(), host_ptr, n * 4);
    } else if (dtype == MI355X_SD_DTYPE_BF16) {
      const uint16_t* s = (const uint16_t*)host_ptr;
      for (int64_t i = 0; i < n; ++i) t.v[i] = bf16_bits_to_f32(s[i]);
    } else if (dtype == MI355X_SD_DTYPE_F16) {
      const uint16_t* s = (const uint16_t*)host_ptr;
      for (int64_t i = 0; i < n; ++i) t.v[i] = f16_bits_to_f32(s[i]);
    } else {
      die(MI355X_SD_ERR_INVALID, "mi355x_sd_unet_load_weight: dtype must be MI355X_SD_DTYPE_F32 / _BF16 / _F16");
    }
    t.loaded = true;
    return MI355X_SD_OK;
  } catch (const std::exception& x) {   // bad_alloc, a malformed number in the config ...: never across the C boundary
    return report(x);
  }
}

int mi355x_sd_unet_weight_bytes(void* handle, size_t* bytes) {
  if (!handle || !bytes) {
    sd::set_last_error("mi355x_sd_unet_weight_bytes: null pointer");
    return MI355X_SD_ERR_INVALID;
  }
  try {
    Exec* e = H_(handle);
    if (!e->packed) {   // (not "host_pack is empty": attach / finalize release the host image, the size stays known)
      for (auto& n : e->order)
        if (!e->params[n].loaded) die(MI355X_SD_ERR_INVALID, "mi355x_sd_unet_weight_bytes: parameter " + n + " was never loaded");
      pack_weights(*e);
      e->packed = true;
    }
    *bytes = e->weight_bytes;
    return MI355X_SD_OK;
  } catch (const std::exception& x) {   // bad_alloc, a malformed number in the config ...: never across the C boundary
    return report(x);
  }
}

int mi355x_sd_unet_pack_weights(void* handle, void* host_buffer, size_t bytes) {
  size_t need = 0;
  const int rc = mi355x_sd_unet_weight_bytes(handle, &need);
  if (rc) return rc;
  Exec* e = H_(handle);
  if (e->host_pack.empty()) {
    sd::set_last_error("mi355x_sd_unet_pack_weights: the packed host image was already released (attach / finalize ran)");
    return MI355X_SD_ERR_INVALID;
  }
  if (!host_buffer || bytes < need) {
    sd::set_last_error("mi355x_sd_unet_pack_weights: buffer missing or too small");
    return MI355X_SD_ERR_INVALID;
  }
  memcpy(host_buffer, e->host_pack.data(), need);
  return MI355X_SD_OK;
}

int mi355x_sd_unet_attach_weights(void* handle, void* device_buffer, size_t bytes) {
  size_t need = 0;
  const int rc = mi355x_sd_unet_weight_bytes(handle, &need);
  if (rc) return rc;
  Exec* e = H_(handle);
  if (!device_buffer || bytes < need || (reinterpret_cast<uintptr_t>(device_buffer) & 255)) {
    sd::set_last_error("mi355x_sd_unet_attach_weights: device buffer missing, too small or not 256-byte aligned");
    return MI355X_SD_ERR_INVALID;
  }
  if (e->dev_w != (unsigned char*)device_buffer) {
    // the plan's launch closures and a captured graph hold ABSOLUTE weight addresses: a moved weight buffer invalidates both
    // (mi355x_sd_unet_plan + _bind_workspace have to run again before the next forward)
    e->drop_graph();
    e->planned = false;
    e->prog_sym.clear();
  }
  e->dev_w = (unsigned char*)device_buffer;
  std::vector<unsigned char>().swap(e->host_pack);
  return MI355X_SD_OK;
}

int mi355x_sd_unet_packed_tensor(void* handle, const char* key, size_t* offset, size_t* bytes, int* rows, int* cols) {
  Exec* e = H_(handle);
  if (!handle || !key || !offset || !bytes || !rows || !cols || e->w.find(key) == e->w.end()) {
    sd::set_last_error("mi355x_sd_unet_packed_tensor: unknown key (pack the weights first)");
    return MI355X_SD_ERR_INVALID;
  }
  const Packed& p = e->w[key];
  *offset = p.off; *bytes = p.bytes; *rows = p.rows; *cols = p.cols;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_finalize_weights(void* handle, void* device_buffer, size_t bytes, void* stream) {
  size_t need = 0;
  const int rc = mi355x_sd_unet_weight_bytes(handle, &need);
  if (rc) return rc;
  Exec* e = H_(handle);
  if (e->host_pack.empty()) {
    sd::set_last_error("mi355x_sd_unet_finalize_weights: the packed host image was already released (attach / finalize ran); "
                       "use mi355x_sd_unet_attach_weights to move to a buffer that already holds the image");
    return MI355X_SD_ERR_INVALID;
  }
  if (!device_buffer || bytes < need || (reinterpret_cast<uintptr_t>(device_buffer) & 255)) {
    sd::set_last_error("mi355x_sd_unet_finalize_weights: device buffer missing, too small or not 256-byte aligned");
    return MI355X_SD_ERR_INVALID;
  }
  if (hipMemcpyAsync(device_buffer, e->host_pack.data(), need, hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(stream)) != hipSuccess ||
      hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) != hipSuccess) {
    sd::set_last_error("mi355x_sd_unet_finalize_weights: host-to-device copy failed");
    return MI355X_SD_ERR_HIP;
  }
  return mi355x_sd_unet_attach_weights(handle, device_buffer, bytes);
}

int mi355x_sd_unet_plan(void* handle, int B, int H, int W, int L, size_t* workspace_bytes) {
  return mi355x_sd_unet_plan_ex(handle, B, H, W, L, 0, workspace_bytes);
}

int mi355x_sd_unet_plan_ex(void* handle, int B, int H, int W, int L, int flags, size_t* workspace_bytes) {
  if (!handle || !workspace_bytes || B <= 0 || H <= 0 || W <= 0 || L <= 0 ||
      (flags & ~(MI355X_SD_UNET_ENC_MASK | MI355X_SD_UNET_SELF_MASK | MI355X_SD_UNET_CONTROLNET))) {
    sd::set_last_error("mi355x_sd_unet_plan: bad argument");
    return MI355X_SD_ERR_INVALID;
  }
  try {
    Exec* e = H_(handle);
    if (!e->dev_w) die(MI355X_SD_ERR_INVALID, "mi355x_sd_unet_plan: call mi355x_sd_unet_finalize_weights first");
    if ((H >> (e->cfg.boc.size() - 1)) < 1 || (W >> (e->cfg.boc.size() - 1)) < 1)
      die(MI355X_SD_ERR_INVALID, "mi355x_sd_unet_plan: latents smaller than one pixel at the lowest level");
    e->drop_graph();
    e->B = B; e->H = H; e->W = W; e->L = L;
    e->plan_flags = flags;
    e->drop_plan();
    e->consts_set = false;
    build_plan(*e);
    e->planned = true;
    *workspace_bytes = e->workspace_bytes;
    return MI355X_SD_OK;
  } catch (const std::exception& x) {   // bad_alloc, a malformed number in the config ...: never across the C boundary
    H_(handle)->drop_plan();   // a failed plan leaves no half-built program behind
    return report(x);
  }
}

int mi355x_sd_unet_bind_workspace(void* handle, void* device_ptr, size_t bytes) {
  Exec* e = H_(handle);
  if (!handle || !e->planned || !device_ptr || bytes < e->workspace_bytes || (reinterpret_cast<uintptr_t>(device_ptr) & 255)) {
    sd::set_last_error("mi355x_sd_unet_bind_workspace: no plan, or buffer missing / too small / not 256-byte aligned");
    return MI355X_SD_ERR_INVALID;
  }
  e->drop_graph();
  e->ws = (unsigned char*)device_ptr;
  e->consts_set = false;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_num_launches(void* handle) { return handle ? (int)H_(handle)->prog_sym.size() : -1; }

// sample [B,Cin,H,W] fp32 NCHW, timestep: one fp32, encoder_hidden_states [B,L,D] fp32, text_embeds [B,text_dim] fp32, time_ids
// [B,6] fp32, out [B,Cout,H,W] fp32 -- all DEVICE pointers (the boundary never touches host memory per step); in_scale: optional
// device scalar multiplied into the sample (the scheduler's scale_model_input), NULL = 1. use_graph != 0: the program is captured
// into a hipGraph on first use with this stream and replayed afterwards.
int mi355x_sd_unet_num_skips(void* handle) { return (handle && H_(handle)->planned) ? (int)H_(handle)->skip_shapes.size() - 1 : -1; }

int mi355x_sd_unet_skip_shape(void* handle, int index, int* C, int* H, int* W) {
  Exec* e = H_(handle);
  if (!handle || !e->planned || !C || !H || !W || index < 0 || index >= (int)e->skip_shapes.size()) {
    sd::set_last_error("mi355x_sd_unet_skip_shape: no plan, or index out of range");
    return MI355X_SD_ERR_INVALID;
  }
  *C = e->skip_shapes[index].C; *H = e->skip_shapes[index].h; *W = e->skip_shapes[index].w;
  return MI355X_SD_OK;
}

int mi355x_sd_unet_set_input(void* handle, const char* name, const void* device_ptr) {
  Exec* e = H_(handle);
  if (!handle || !name) {
    sd::set_last_error("mi355x_sd_unet_set_input: null handle or name");
    return MI355X_SD_ERR_INVALID;
  }
  const std::string n(name);
  if (n == "class_labels") {
    if (e->cfg.class_kind == Cfg::CLASS_NONE && device_ptr) {
      // (the reference ignores class_labels on a model without a class embedding, unet_2d_condition.py:953; a binding that
      // nothing will ever read is more likely a wrong handle than intent)
      sd::set_last_error("mi355x_sd_unet_set_input: this model has no class embedding");
      return MI355X_SD_ERR_INVALID;
    }
    e->class_ptr = device_ptr;
    return MI355X_SD_OK;
  }
  if (n == "timestep_cond") {
    if (!e->cfg.tcp && device_ptr) {
      sd::set_last_error("mi355x_sd_unet_set_input: timestep_cond was passed but the model has no `time_cond_proj_dim`");
      return MI355X_SD_ERR_INVALID;
    }
    e->tcond_ptr = static_cast<const float*>(device_ptr);
    return MI355X_SD_OK;
  }
  if (n == "image_embeds") {
    if (!e->cfg.ip && device_ptr) {
      sd::set_last_error("mi355x_sd_unet_set_input: this model has no IP-Adapter (config encoder_hid_dim_type != 'ip_image_proj')");
      return MI355X_SD_ERR_INVALID;
    }
    e->image_ptr = static_cast<const float*>(device_ptr);
    return MI355X_SD_OK;
  }
  sd::set_last_error(("mi355x_sd_unet_set_input: unknown input '" + n + "' (class_labels, timestep_cond, image_embeds)").c_str());
  return MI355X_SD_ERR_INVALID;
}

int mi355x_sd_unet_forward(void* handle, void* stream, const float* sample, const float* timestep, const float* encoder_hidden_states,
                           const float* text_embeds, const float* time_ids, const float* in_scale, float* out, int use_graph) {
  return mi355x_sd_unet_forward_ex(handle, stream, sample, timestep, encoder_hidden_states, text_embeds, time_ids, in_scale, nullptr,
                                   nullptr, nullptr, 0, nullptr, out, use_graph);
}

int mi355x_sd_unet_forward_ex(void* handle, void* stream, const float* sample, const float* timestep, const float* encoder_hidden_states,
                              const float* text_embeds, const float* time_ids, const float* in_scale,
                              const float* encoder_attention_mask, const float* attention_mask,
                              const float* const* down_block_additional_residuals, int num_down_residuals,
                              const float* mid_block_additional_residual, float* out, int use_graph) {
  Exec* e = H_(handle);
  if (!handle || !e->planned || !e->ws) {
    sd::set_last_error("mi355x_sd_unet_forward: plan and bind a workspace first");
    return MI355X_SD_ERR_INVALID;
  }
  if (!sample || !timestep || !encoder_hidden_states || !out) {
    sd::set_last_error("mi355x_sd_unet_forward: null pointer");
    return MI355X_SD_ERR_INVALID;
  }
  if (e->cfg.text_time && (!text_embeds || !time_ids)) {
    // the reference raises ValueError here (unet_2d_condition.py:993-1001)
    sd::set_last_error("mi355x_sd_unet_forward: addition_embed_type 'text_time' requires text_embeds and time_ids");
    return MI355X_SD_ERR_INVALID;
  }
  if (e->cfg.ip && !e->image_ptr) {
    // unet_2d_condition.py:1055-1058
    sd::set_last_error("mi355x_sd_unet_forward: encoder_hid_dim_type 'ip_image_proj' requires image_embeds (mi355x_sd_unet_set_input)");
    return MI355X_SD_ERR_INVALID;
  }
  if (e->cfg.class_kind != Cfg::CLASS_NONE && !e->class_ptr) {
    // unet_2d_condition.py:954-955
    sd::set_last_error("mi355x_sd_unet_forward: class_labels should be provided when num_class_embeds > 0 (mi355x_sd_unet_set_input)");
    return MI355X_SD_ERR_INVALID;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Cfg& c = e->cfg;
  const int B = e->B, H = e->H, W = e->W, L = e->L;
  // ---- the optional inputs must be exactly the ones the plan was built for ----
  const bool want_enc = (e->plan_flags & MI355X_SD_UNET_ENC_MASK) != 0, want_self = (e->plan_flags & MI355X_SD_UNET_SELF_MASK) != 0;
  const bool want_ctrl = (e->plan_flags & MI355X_SD_UNET_CONTROLNET) != 0;
  const bool has_ctrl = down_block_additional_residuals != nullptr || mid_block_additional_residual != nullptr;
  if (want_enc != (encoder_attention_mask != nullptr) || want_self != (attention_mask != nullptr) || want_ctrl != has_ctrl) {
    sd::set_last_error("mi355x_sd_unet_forward_ex: optional inputs differ from the plan's flags (mi355x_sd_unet_plan_ex)");
    return MI355X_SD_ERR_INVALID;
  }
  if (want_ctrl) {
    if (!down_block_additional_residuals || !mid_block_additional_residual) {
      // down residuals alone are the reference's deprecated T2I-Adapter form (unet_2d_condition.py:1084-1094): the intrablock adds
      // are planned by the Python planner only (paddlemix_amd.unet), not by this handle
      sd::set_last_error("mi355x_sd_unet_forward_ex: ControlNet residuals need both down_block_additional_residuals and "
                         "mid_block_additional_residual; T2I-Adapter (intrablock) residuals are not supported by the C handle");
      return MI355X_SD_ERR_UNSUPPORTED;
    }
    if (num_down_residuals != (int)e->ctrl_down.size()) {
      sd::set_last_error("mi355x_sd_unet_forward_ex: wrong number of down_block_additional_residuals (mi355x_sd_unet_num_skips)");
      return MI355X_SD_ERR_INVALID;
    }
    for (int i = 0; i < num_down_residuals; ++i)
      if (!down_block_additional_residuals[i]) {
        sd::set_last_error("mi355x_sd_unet_forward_ex: null residual pointer");
        return MI355X_SD_ERR_INVALID;
      }
  }
  // ---- stage inputs into the plan's static buffers (device-to-device, stream ordered) ----
  auto staging_failed = [] {
    sd::set_last_error("mi355x_sd_unet_forward: staging copy failed");
    return (int)MI355X_SD_ERR_HIP;
  };
  bool ok = hipMemcpyAsync(e->at(e->in_sample), sample, (size_t)4 * B * c.in_channels * H * W, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (want_enc) ok = ok && hipMemcpyAsync(e->at(e->enc_mask), encoder_attention_mask, (size_t)4 * B * L, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (want_self) ok = ok && hipMemcpyAsync(e->at(e->self_mask), attention_mask, (size_t)4 * B * H * W, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (want_ctrl) {
    for (size_t i = 0; i < e->ctrl_down.size(); ++i) {
      const Exec::SkipShape& sk = e->skip_shapes[i];
      ok = ok && hipMemcpyAsync(e->at(e->ctrl_down[i]), down_block_additional_residuals[i], (size_t)4 * B * sk.C * sk.h * sk.w,
                                hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    const Exec::SkipShape& mk = e->skip_shapes.back();
    ok = ok && hipMemcpyAsync(e->at(e->ctrl_mid), mid_block_additional_residual, (size_t)4 * B * mk.C * mk.h * mk.w, hipMemcpyDeviceToDevice,
                              st) == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(e->at(e->in_t), timestep, 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (in_scale) {
    ok = ok && hipMemcpyAsync(e->at(e->in_scale), in_scale, 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    e->consts_set = false;
  } else if (!e->consts_set) {
    static const float one = 1.0f;
    ok = ok && hipMemcpyAsync(e->at(e->in_scale), &one, 4, hipMemcpyHostToDevice, st) == hipSuccess;
    e->consts_set = true;
  }
  if (!ok) return staging_failed();
  int rc = mi355x_sd_cast_rows(encoder_hidden_states, c.cross_dim, e->at(e->in_enc), c.cross_dim, (int64_t)B * L, c.cross_dim, stream);
  if (rc) return rc;
  if (c.ip) {
    rc = mi355x_sd_cast_rows(e->image_ptr, c.ehd, e->at(e->in_image), c.ehd, B, c.ehd, stream);
    if (rc) return rc;
  }
  if (c.tcp) {
    if (e->tcond_ptr) {
      rc = mi355x_sd_cast_rows(e->tcond_ptr, c.tcp, e->at(e->in_tcond), c.tcp, B, c.tcp, stream);
      if (rc) return rc;
    } else if (hipMemsetAsync(e->at(e->in_tcond), 0, (size_t)2 * B * c.tcp, st) != hipSuccess) return staging_failed();
  }
  if (c.class_kind == Cfg::CLASS_TABLE || c.class_kind == Cfg::CLASS_TIMESTEP) {   // int32 indices / fp32 values, one per sample
    if (hipMemcpyAsync(e->at(e->in_class), e->class_ptr, (size_t)4 * B, hipMemcpyDeviceToDevice, st) != hipSuccess) return staging_failed();
  } else if (c.class_kind != Cfg::CLASS_NONE) {
    const int wdt = c.class_kind == Cfg::CLASS_IDENTITY ? c.boc[0] * 4 : c.pdim;
    rc = mi355x_sd_cast_rows((const float*)e->class_ptr, wdt, e->at(e->in_class), wdt, B, wdt, stream);
    if (rc) return rc;
  }
  if (c.text_time) {
    rc = mi355x_sd_cast_rows(text_embeds, e->text_dim, e->at(e->in_addin), c.pdim, B, e->text_dim, stream);
    if (rc) return rc;
    if (hipMemcpyAsync(e->at(e->in_tids), time_ids, (size_t)4 * B * e->n_ids, hipMemcpyDeviceToDevice, st) != hipSuccess) return staging_failed();
  }
  // ---- the program ----
  auto run_eager = [&]() {
    for (auto& f : e->prog_sym) {
      const int r = f(stream);
      if (r) return r;
    }
    return (int)MI355X_SD_OK;
  };
  if (use_graph) {
    if (!e->graph || e->graph_stream != stream) {
      e->drop_graph();
      rc = run_eager();   // warm-up outside capture (lazy module loading), also this call's result
      if (rc) return rc;
      rc = mi355x_sd_graph_begin(stream);
      if (rc) return rc;
      const int rprog = run_eager();
      void* exec = nullptr;
      rc = mi355x_sd_graph_end(stream, &exec);
      if (rprog || rc) {   // a launch failed inside the capture: do not keep (or leak) the partial graph
        if (exec) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(exec));
        return rprog ? rprog : rc;
      }
      e->graph = reinterpret_cast<hipGraphExec_t>(exec);
      e->graph_stream = stream;
    } else {
      rc = mi355x_sd_graph_launch(e->graph, stream);
      if (rc) return rc;
    }
  } else {
    rc = run_eager();
    if (rc) return rc;
  }
  if (hipMemcpyAsync(out, e->at(e->out), (size_t)4 * B * c.out_channels * H * W, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    sd::set_last_error("mi355x_sd_unet_forward: output copy failed");
    return MI355X_SD_ERR_HIP;
  }
  return MI355X_SD_OK;
}

}  // extern "C"
