// Internal types of the U-Net handle (seam B1): what unet_config.hip, unet_weights.hip, unet_plan.hip and unet_exec.hip share.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mi355x_sd.h"
#include "common.h"
#include "kernels.h"

namespace sd {
namespace unet {

// ---------------------------------------------------------------------------------------------------------------- errors
struct ExecError : std::runtime_error {
  int code;
  ExecError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void die(int code, const std::string& m) { throw ExecError(code, m); }

// ---------------------------------------------------------------------------------------------------------------- config
struct Cfg {
  int in_channels = 4, out_channels = 4;
  bool flip_sin_to_cos = true;
  double freq_shift = 0.0;
  std::vector<std::string> down = {"CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"};
  std::vector<std::string> up = {"UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"};
  std::vector<int> boc = {320, 640, 1280, 1280};
  std::vector<int> layers_per_block, tlayers, heads;
  int cross_dim = 1280;
  double mid_scale = 1.0;
  int groups = 32;
  double norm_eps = 1e-5;
  bool linear_proj = false;
  bool text_time = false;
  int atd = 0, pdim = 0;
  // class embedding (unet_2d_condition.py:404-441, 953-975) and TimestepEmbedding.cond_proj (embeddings.py:265-266, 284-285)
  enum ClassKind { CLASS_NONE, CLASS_TABLE, CLASS_TIMESTEP, CLASS_IDENTITY, CLASS_PROJECTION, CLASS_SIMPLE };
  ClassKind class_kind = CLASS_NONE;
  int num_class = 0;      // rows of the nn.Embedding table (CLASS_TABLE)
  int tcp = 0;            // time_cond_proj_dim (0: none)
  bool concat = false;    // class_embeddings_concat: the blocks see [emb | class_emb] (blocks_time_embed_dim = 2 x time_embed_dim, :443-449)
  // IP-Adapter (encoder_hid_dim_type "ip_image_proj": ImageProjection embeddings.py:507-518 + IPAdapterAttnProcessor on every attn2)
  bool ip = false;
  int ehd = 0, ip_tokens = 4;   // encoder_hid_dim; ImageProjection.num_image_text_embeds (extension key ip_adapter_num_tokens, as unet.py)
};

// ---------------------------------------------------------------------------------------------------------------- structure
struct Layer {
  enum Kind { SKIP, RESNET, ATTN, DOWN, UP, CAT } kind;
  std::string name;
  int cin = 0, cout = 0;   // RESNET: cin -> cout; ATTN / DOWN / UP: channels in cout; CAT: skip channels in cout
  double scale = 1.0;
  int heads = 0, layers = 0;
};

// ---------------------------------------------------------------------------------------------------------------- weights
struct HostT {
  std::vector<int64_t> shape;
  std::vector<float> v;
  bool loaded = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    return n;
  }
};

struct Packed {   // one packed device tensor: offset into the weight buffer
  size_t off = 0, bytes = 0;
  int rows = 0, cols = 0;   // [N][K] for matrices
};

// symbolic workspace address
struct Ref {
  int buf = -1;   // index into Exec::bufs; -1: absolute (weights / null)
  size_t off = 0;
  const void* abs = nullptr;
};
struct View {   // rows x C elements of `es` bytes, row stride ld elements
  Ref p;
  int rows = 0, C = 0, ld = 0, es = 2;
  View cols(int off, int c) const {
    View v = *this;
    v.p.off += (size_t)off * es;
    v.C = c;
    return v;
  }
};

struct Exec {
  Cfg cfg;
  std::vector<Layer> layers;
  std::map<std::string, HostT> params;            // expected parameters (reference names, Paddle layouts)
  std::vector<std::string> order;                 // construction order
  bool resid_f32 = false;
  bool fold_scale = true;                         // head_dim^-0.5 * log2(e) folded into the self-attention to_q weights (head_dim 64)
  std::set<std::string> log2_blocks;
  // packed weights
  std::map<std::string, Packed> w;
  std::vector<unsigned char> host_pack;
  bool packed = false;        // Packer ran (it consumes the loaded fp32 tensors: it must never run twice)
  size_t weight_bytes = 0;
  unsigned char* dev_w = nullptr;
  std::map<std::string, int> temb_off, kv_off;
  std::set<std::string> kb64;                     // 3x3 convs whose weights are packed in 64-channel blocks
  int temb_total = 0, kv_total = 0;
  // plan
  int B = 0, H = 0, W = 0, L = 0;
  struct Buf {
    std::string name;
    size_t bytes = 0, off = 0;
  };
  std::vector<Buf> bufs;
  std::map<std::string, int> buf_index;
  size_t workspace_bytes = 0;
  unsigned char* ws = nullptr;
  std::vector<std::function<int(void*)>> prog_sym;   // built at plan time, read `ws` at run time
  Ref in_sample, in_t, in_scale, in_enc, in_addin, in_tids, out;
  Ref in_class, in_tcond, in_image;               // class_labels / timestep_cond / image_embeds as the program reads them (mi355x_sd_unet_set_input)
  const float* image_ptr = nullptr;
  float ip_scale = 1.0f;                          // IPAdapterAttnProcessor.scale (mi355x_sd_unet_set_ip_adapter_scale; a launch constant of the plan)
  bool freeu = false;                             // FreeU (mi355x_sd_unet_set_freeu): launch constants of the plan, like ip_scale
  float freeu_s[2] = {1.0f, 1.0f}, freeu_b[2] = {1.0f, 1.0f};   // (s1, s2), (b1, b2): up blocks 0 and 1
  const void* class_ptr = nullptr;                // caller's device tensors, read by every forward call until replaced
  const float* tcond_ptr = nullptr;
  // optional inputs chosen at plan time (mi355x_sd_unet_plan_ex flags)
  int plan_flags = 0;
  Ref enc_mask, enc_bias, self_mask, self_bias, ctrl_mid;
  std::vector<Ref> ctrl_down;
  struct SkipShape { int C, h, w; };
  std::vector<SkipShape> skip_shapes;             // every skip tensor, then the mid block's output
  int text_dim = 0, n_ids = 0;
  bool planned = false, consts_set = false;
  hipGraphExec_t graph = nullptr;
  void* graph_stream = nullptr;

  void* at(const Ref& r) const { return r.buf < 0 ? const_cast<void*>(r.abs) : (void*)(ws + bufs[r.buf].off + r.off); }
  void drop_graph() {   // a captured graph holds the addresses of the plan and the buffers it was captured with
    if (graph) (void)hipGraphExecDestroy(graph);
    graph = nullptr;
  }
  void drop_plan() {
    planned = false;
    prog_sym.clear();
    bufs.clear();
    buf_index.clear();
    skip_shapes.clear();
    ctrl_down.clear();
    ws = nullptr;
  }
};

Cfg parse_config(const char* json);          // unet_config.hip
std::vector<Layer> structure(const Cfg& c);
void build_param_table(Exec& e);             // unet_weights.hip
void pack_weights(Exec& e);
void build_plan(Exec& e);                    // unet_plan.hip

}  // namespace unet
}  // namespace sd
