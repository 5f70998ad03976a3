// Host-only dump of the C++ U-Net planner (paddlemix_amd/csrc/unet_*.hip): every launch of a plan with every argument, and the packed
// weight image, as text that two checkouts can be diffed by. Nothing runs on a GPU: the planner's translation units are #included, the
// mi355x_sd_* entry points its closures call are recording stand-ins defined here, and the weight / workspace bases are fake addresses
// that are only ever subtracted again. scripts/compare_unet_plans.py builds this against a csrc directory and walks the case grid.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -I <csrc> scripts/c/unet_plan_dump.cpp -o unet_plan_dump
//   unet_plan_dump config.json image.bin B,H,W,L,flags,resid_f32[,freeu] [B,H,W,L,flags,resid_f32[,freeu] ...]
// (freeu = 1: the plan with FreeU on, s1 = 0.9, s2 = 0.2, b1 = 1.3, b2 = 1.4; a checkout from before ABI 22 prints an error line for it)
#if __has_include("unet_plan.hip")
#include "unet_config.hip"
#include "unet_weights.hip"
#include "unet_plan.hip"
#include "unet_exec.hip"
#else   // a checkout from before the file was split
#include "unet_exec.hip"
#endif
#include <fstream>
#include <sstream>
#include <type_traits>

static char g_last[2048];
namespace sd { namespace unet {} void set_last_error(const char* m) { snprintf(g_last, sizeof(g_last), "%s", m ? m : ""); } }
using namespace sd::unet;

static unsigned char* const WBASE = reinterpret_cast<unsigned char*>(0x100000000000ull);   // weights
static unsigned char* const SBASE = reinterpret_cast<unsigned char*>(0x200000000000ull);   // workspace
static size_t g_wbytes, g_sbytes;

static void put(const void* p) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  if (!p) printf(" null");
  else if (c >= WBASE && c < WBASE + g_wbytes) printf(" W+%zu", (size_t)(c - WBASE));
  else if (c >= SBASE && c < SBASE + g_sbytes) printf(" S+%zu", (size_t)(c - SBASE));
  else printf(" ?%p", p);
}
template <class T>
static std::enable_if_t<std::is_arithmetic<T>::value> put(T v) {
  if (std::is_floating_point<T>::value) printf(" %.9g", (double)v);
  else printf(" %lld", (long long)v);
}
template <class... A>
static int rec(const char* sym, A... a) {
  printf("%s", sym);
  (put(a), ...);
  printf("\n");
  return 0;
}

typedef const void* CV;
typedef const float* CF;
typedef int64_t I8;
extern "C" {
// plan-time queries: the documented fit rule of the one-launch GroupNorm, and a workspace size of the real one's shape
int mi355x_sd_groupnorm_act_fits(int HW, int C, int g) { return g > 0 && C % g == 0 && !((C / g) & 1) && C / g <= 128 && (long)HW * (C / g) * 2 <= 96 << 10; }
int mi355x_sd_groupnorm_workspace_floats(int B, int HW, int C) { return 2 * B * C * ((HW + 1023) / 1024); }
int mi355x_sd_graph_begin(void*) { return 0; }
int mi355x_sd_graph_end(void*, void**) { return 0; }
int mi355x_sd_graph_launch(void*, void*) { return 0; }
int mi355x_sd_linear(CV a, int lda, CV w, void* c, int ldc, int M, int N, int K, CF b, CF rb, int rpb, int ldrb, CV R, int ldr, float os, int fl,
                     void* ws, size_t wsb, void* st) { return rec("linear", a, lda, w, c, ldc, M, N, K, b, rb, rpb, ldrb, R, ldr, os, fl, ws, wsb, st); }
int mi355x_sd_conv3x3(CV x, int ldx, int B, int H, int W, int Ci, int s, int up, CV w, void* c, int ldc, int Co, CF b, CF rb, int ldrb, CV R,
                      int ldr, float os, int fl, void* ws, size_t wsb, void* st) {
  return rec("conv3x3", x, ldx, B, H, W, Ci, s, up, w, c, ldc, Co, b, rb, ldrb, R, ldr, os, fl, ws, wsb, st);
}
#define SDPA_ARGS CV q, CV k, CV v, CF bias, void* o, int B, int H, int Sq, int Skv, int D, I8 qb, int qt, I8 kb, int kt, I8 vb, int vt, I8 ob, int ot, I8 b0, I8 b1, I8 b2, float sc
#define SDPA_VALS q, k, v, bias, o, B, H, Sq, Skv, D, qb, qt, kb, kt, vb, vt, ob, ot, b0, b1, b2, sc
int mi355x_sd_sdpa(SDPA_ARGS, void* st) { return rec("sdpa", SDPA_VALS, st); }
int mi355x_sd_sdpa_ex(SDPA_ARGS, int fl, void* st) { return rec("sdpa_ex", SDPA_VALS, fl, st); }
int mi355x_sd_sdpa_accum(SDPA_ARGS, float os, void* st) { return rec("sdpa_accum", SDPA_VALS, os, st); }
int mi355x_sd_groupnorm_act(CV x, int B, int HW, int C, int ldx, int g, float eps, CF ga, CF be, int silu, void* y, int ldy, void* st) {
  return rec("groupnorm_act", x, B, HW, C, ldx, g, eps, ga, be, silu, y, ldy, st);
}
int mi355x_sd_groupnorm_stats_ex(CV x, int B, int HW, int C, int ldx, int g, float eps, CF ga, CF be, float* ws, float* ss, int f32, void* st) {
  return rec("groupnorm_stats_ex", x, B, HW, C, ldx, g, eps, ga, be, ws, ss, f32, st);
}
int mi355x_sd_scale_shift_act_ex(CV x, int B, int HW, int C, int ldx, CF ss, int silu, void* y, int ldy, int f32, void* raw, int ldraw, void* st) {
  return rec("scale_shift_act_ex", x, B, HW, C, ldx, ss, silu, y, ldy, f32, raw, ldraw, st);
}
int mi355x_sd_layernorm_ex(CV x, int rows, int C, int ldx, CF g, CF b, float eps, void* y, int ldy, int f32, void* st) {
  return rec("layernorm_ex", x, rows, C, ldx, g, b, eps, y, ldy, f32, st);
}
int mi355x_sd_cast_rows(CF x, int ldx, void* y, int ldy, I8 rows, int C, void* st) { return rec("cast_rows", x, ldx, y, ldy, rows, C, st); }
int mi355x_sd_copy_rows(CV x, int ldx, void* y, int ldy, I8 rows, int C, void* st) { return rec("copy_rows", x, ldx, y, ldy, rows, C, st); }
int mi355x_sd_timestep_embedding(CF t, int tc, int n, int dim, int grp, int flip, float fs, float sc, float mp, void* o, int ldo, void* st) {
  return rec("timestep_embedding", t, tc, n, dim, grp, flip, fs, sc, mp, o, ldo, st);
}
int mi355x_sd_embed_tokens(const int32_t* ids, I8 n, int seq, CV tab, CV pos, int D, void* o, int ldo, void* st) {
  return rec("embed_tokens", (CV)ids, n, seq, tab, pos, D, o, ldo, st);
}
int mi355x_sd_silu(CV x, void* y, I8 n, int inf, int outf, void* st) { return rec("silu", x, y, n, inf, outf, st); }
int mi355x_sd_mask_to_bias(CF m, float* b, I8 n, void* st) { return rec("mask_to_bias", m, b, n, st); }
int mi355x_sd_conv_in3x3_ex(CF x, CF s, CV w, CF b, void* y, int B, int Ci, int H, int W, int Co, int ldy, int f32, void* st) {
  return rec("conv_in3x3_ex", x, s, w, b, y, B, Ci, H, W, Co, ldy, f32, st);
}
int mi355x_sd_conv_out3x3(CV x, int ldx, CV w, CF b, float* y, int B, int Ci, int H, int W, int Co, void* st) {
  return rec("conv_out3x3", x, ldx, w, b, y, B, Ci, H, W, Co, st);
}
int mi355x_sd_add_nchw_ex(void* x, int ldx, CF r, int B, int C, I8 HW, int f32, void* st) { return rec("add_nchw_ex", x, ldx, r, B, C, HW, f32, st); }
#if MI355X_SD_ABI_VERSION >= 22
I8 mi355x_sd_freeu_workspace_floats(int B, int H, int W, int Cs) { return sd::freeu_workspace_floats(B, H, W, Cs); }   // the library's own (kernels.h)
int mi355x_sd_freeu(void* cat, I8 ld, int B, int H, int W, int Cx, int Cs, float b, float s, int f32, float* ws, void* st) {
  return rec("freeu", cat, ld, B, H, W, Cx, Cs, b, s, f32, (CV)ws, st);
}
#endif
}

#define CHECK(call)                                                        \
  if (int rc_ = (call)) {                                                  \
    printf("error %d: %s\n", rc_, g_last);                                 \
    return 0;                                                              \
  }

static int run(int argc, char** argv) {
  std::stringstream json;
  json << std::ifstream(argv[1]).rdbuf();
  void* h = nullptr;
  CHECK(mi355x_sd_unet_create(json.str().c_str(), &h));
  Exec* e = reinterpret_cast<Exec*>(h);
  uint32_t lcg = 12345u;   // the same pseudo-random weights for every checkout, roughly N(0, 1/16)-sized
  std::vector<float> buf;
  for (int i = 0; i < mi355x_sd_unet_num_params(h); ++i) {
    const char* name;
    int64_t shape[4];
    int nd;
    CHECK(mi355x_sd_unet_param_info(h, i, &name, shape, &nd));
    buf.resize((size_t)(shape[0] * shape[1] * shape[2] * shape[3]));
    for (float& v : buf) v = (float)(int32_t)(lcg = lcg * 1664525u + 1013904223u) * (0.25f / 2147483648.0f);
    CHECK(mi355x_sd_unet_load_weight(h, name, buf.data(), shape, nd, MI355X_SD_DTYPE_F32));
  }
  CHECK(mi355x_sd_unet_weight_bytes(h, &g_wbytes));
  std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char*>(e->host_pack.data()), (std::streamsize)e->host_pack.size());
  for (auto& kv : e->w) printf("packed %s off=%zu bytes=%zu rows=%d cols=%d\n", kv.first.c_str(), kv.second.off, kv.second.bytes, kv.second.rows, kv.second.cols);
  CHECK(mi355x_sd_unet_attach_weights(h, WBASE, g_wbytes));
  for (int a = 3; a < argc; ++a) {
    int B, H, W, L, flags, f32, freeu = 0;
    if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d", &B, &H, &W, &L, &flags, &f32, &freeu) < 6) return 2;
    printf("plan %s\n", argv[a]);
    e->resid_f32 = f32 != 0;
#if MI355X_SD_ABI_VERSION >= 22
    CHECK(mi355x_sd_unet_set_freeu(h, freeu, 0.9f, 0.2f, 1.3f, 1.4f));
#else
    if (freeu) {
      printf("error: this checkout has no FreeU\n");
      continue;
    }
#endif
    if (int rc = mi355x_sd_unet_plan_ex(h, B, H, W, L, flags, &g_sbytes)) {
      printf("error %d: %s\n", rc, g_last);
      continue;
    }
    e->ws = SBASE;
    printf("workspace %zu launches %zu\n", g_sbytes, e->prog_sym.size());
    for (auto& b : e->bufs) printf("buf %s off=%zu bytes=%zu\n", b.name.c_str(), b.off, b.bytes);
    for (auto& f : e->prog_sym) f(nullptr);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  return run(argc, argv);
}
