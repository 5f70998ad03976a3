// C ABI of libmi355x_sd.so (declared in include/mi355x_sd.h): argument validation + kernel launches.
#include "../../include/mi355x_sd.h"

#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "common.h"
#include "kernels.h"

namespace {
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, const char* a = "") {
  snprintf(g_err, sizeof(g_err), fmt, a);
  return code;
}
int finish(int rc, const char* what) {
  if (rc == SD_OK) return SD_OK;
  if (rc == SD_ERR_HIP) {
    hipError_t e = hipGetLastError();
    snprintf(g_err, sizeof(g_err), "%s: HIP error: %s", what, hipGetErrorString(e));
  } else if (rc == SD_ERR_UNSUPPORTED) {
    snprintf(g_err, sizeof(g_err), "%s: unsupported shape/stride/alignment (see include/mi355x_sd.h)", what);
  } else {
    snprintf(g_err, sizeof(g_err), "%s: invalid argument", what);
  }
  return rc;
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace

namespace sd {
void set_last_error(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }
}  // namespace sd

using namespace sd;

// ---- layout probe (tests/test_gpu_probe.py) -------------------------------------------------------------------
__global__ void probe_kernel(float* out) {
  __shared__ __attribute__((aligned(16))) bf16 lds[256];
  const int l = threadIdx.x;
  for (int i = l; i < 256; i += 64) lds[i] = (bf16)(float)i;
  __syncthreads();
  // 16x16x32: a lane supplies A[row = l&15][k = (l>>4)*8 + i], B[k = (l>>4)*8 + i][col = l&15]
  bf16x8 a, b;
  for (int i = 0; i < 8; ++i) {
    const int k = (l >> 4) * 8 + i;
    a[i] = (bf16)(float)((((l & 15) * 7 + k * 3) % 11) - 5);
    b[i] = (bf16)(float)(((k * 5 + (l & 15) * 2) % 13) - 6);
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = mfma_16x16x32(a, b, c);
  for (int i = 0; i < 4; ++i) out[l * 24 + i] = c[i];
  // 32x32x16: A[row = l&31][k = (l>>5)*8 + i], B[k][col = l&31]
  for (int i = 0; i < 8; ++i) {
    const int k = (l >> 5) * 8 + i;
    a[i] = (bf16)(float)((((l & 31) * 7 + k * 3) % 11) - 5);
    b[i] = (bf16)(float)(((k * 5 + (l & 31) * 2) % 13) - 6);
  }
  f32x16 d;
  for (int i = 0; i < 16; ++i) d[i] = 0.f;
  d = mfma_32x32x16(a, b, d);
  for (int i = 0; i < 16; ++i) out[l * 24 + 4 + i] = d[i];
  const bf16x4 t = ds_read_tr16((lds_bf16x4*)(lds + l * 4));
  for (int i = 0; i < 4; ++i) out[l * 24 + 20 + i] = (float)t[i];
}

// Scratch argument of the GEMM-class entry points (ABI 12): NULL or 16-byte aligned DEVICE memory. A host pointer is refused here, not
// at the first split-K launch that writes through it (round 5: a host buffer bound on a misuse path killed a later launch with a page
// fault on a box without XNACK). The runtime query sits on every GEMM launch, so the last accepted (pointer, size) is remembered per
// thread and not asked about again; a pointer the runtime cannot classify (hipErrorInvalidValue: plain malloc memory on some ROCm
// releases, unregistered ranges) is NOT device memory as far as this library can tell and is refused as well.
static int check_ws(const void* ws, size_t bytes, const char* who) {
  if (!ws) return SD_OK;
  if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(SD_ERR_INVALID, "%s: the workspace pointer must be 16-byte aligned", who);
  static thread_local const void* ok_ptr = nullptr;
  static thread_local size_t ok_bytes = 0;
  if (ws == ok_ptr && bytes <= ok_bytes) return SD_OK;
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, ws);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(SD_ERR_INVALID, "%s: the workspace must be device memory (the HIP runtime does not know this pointer)", who);
  }
  if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)
    return fail(SD_ERR_INVALID, "%s: the workspace must be device memory", who);
  ok_ptr = ws;
  ok_bytes = bytes;
  return SD_OK;
}

// The GemmArgs of the six GEMM-class entries, stated once: gemm_args() zeroes the struct (a field an entry does not name is off) and sets
// what all six share -- the scratch pair of an entry that takes one included, which that entry has passed through check_ws() -- and
// epilogue_flags() decodes the flag bits the entry honours. An entry then states only what is its own.
static GemmArgs gemm_args(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K, void* ws = nullptr,
                          size_t ws_bytes = 0) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = (const bf16*)A; g.W = (const bf16*)W; g.C = C;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc;
  g.ws_base = ws; g.ws_bytes = ws ? ws_bytes : 0;
  return g;
}
constexpr int EPILOGUE_CONV = MI355X_SD_OUT_F32 | MI355X_SD_R_F32 | MI355X_SD_SILU;   // (GEGLU is refused there, GELU_TANH not honoured)
constexpr int EPILOGUE_LINEAR = EPILOGUE_CONV | MI355X_SD_GEGLU;                       // (mi355x_sd_linear: GELU_TANH not honoured)
constexpr int EPILOGUE_ALL = EPILOGUE_LINEAR | MI355X_SD_GELU_TANH;
static void epilogue_flags(GemmArgs& g, int flags, int honoured) {
  flags &= honoured;
  g.geglu = (flags & MI355X_SD_GEGLU) ? 1 : 0;
  g.out_f32 = (flags & MI355X_SD_OUT_F32) ? 1 : 0;
  g.r_f32 = (flags & MI355X_SD_R_F32) ? 1 : 0;
  g.silu = (flags & MI355X_SD_SILU) ? 1 : 0;
  g.gelu_tanh = (flags & MI355X_SD_GELU_TANH) ? 1 : 0;
}

// The argument rule of the step-tail entries (step_tail.hip), stated once: step_entry() checks a call against its operands and
// launches. An entry names its operands in the header's order -- paddlemix_amd/step_forms.py holds the same row for the Python side,
// tests/test_step_forms.py generates every refusal from it. Blocks write their part of the written spans while other blocks still read
// the inputs, so a written span must not overlap another one, nor anything read -- except the read operand named by `same`, when the
// two are one pointer: the same lane reads and then writes each element of such a pair. A null span (no guidance, no noise) overlaps
// nothing. The range: batch > 0, per_sample >= 1 (>= 2 under the rescale), and batch * per_sample * planes * 4 bytes fit an int64_t
// for the operand of the most planes; a span's length is meaningful only once the range has passed, and only then is it used.
struct StepOperand {
  const char* name;
  const void* p;
  int planes;      // the span is planes * batch * per_sample floats
  bool written;
  bool optional;   // may be null
  int same;        // written: the index of the read operand it may be itself, or -1
};
static StepOperand reads(const char* name, const void* p, bool optional = false) { return {name, p, 1, false, optional, -1}; }
static StepOperand writes(const char* name, const void* p, int planes = 1, int same = -1) { return {name, p, planes, true, false, same}; }
struct StepCoef {
  const float* p;
  int floats, align;   // the row and the alignment its loads need, in bytes
  bool overlaps;       // takes part in the overlap rule
};

// always_rescale (cfg_rescale_axpby): the rescale runs whatever guidance_rescale is, which goes to the launch as it came; otherwise
// the launch gets 0 unless there is an eps_text to rescale by. launch(guidance_rescale) -> the launcher's status
template <class Launch>
static int step_entry(const char* who, std::initializer_list<StepOperand> operands, StepCoef coef, const float* eps_text,
                      float guidance_rescale, bool always_rescale, int batch, int64_t per_sample, Launch launch) {
  auto refuse = [who](const char* rule, const char* a = "", const char* b = "") {
    snprintf(g_err, sizeof(g_err), rule, who, a, b);
    return (int)SD_ERR_INVALID;
  };
  int planes = 1;
  for (const StepOperand& o : operands) {
    if (!o.p && !o.optional) return refuse("%s: null pointer (%s)", o.name);
    planes = o.planes > planes ? o.planes : planes;
  }
  if (!coef.p) return refuse("%s: null pointer (%s)", "coef");
  if ((uintptr_t)coef.p % (uintptr_t)coef.align) {
    snprintf(g_err, sizeof(g_err), "%s: coef must be %d-byte aligned", who, coef.align);
    return SD_ERR_INVALID;
  }
  const bool rescale = always_rescale || (eps_text && guidance_rescale > 0.0f);
  if (batch <= 0 || per_sample < (rescale ? 2 : 1) || per_sample > INT64_MAX / 4 / planes / batch)
    return refuse(always_rescale ? "%s: needs batch > 0 and per_sample >= 2 (the estimator divides by per_sample - 1)"
                                 : "%s: needs batch > 0 and per_sample >= 1 (>= 2 with guidance_rescale: the estimator divides by "
                                   "per_sample - 1)");
  const uintptr_t bytes = (uintptr_t)batch * (uintptr_t)per_sample * 4;
  auto overlap = [](const void* a, uintptr_t la, const void* b, uintptr_t lb) {
    return a && b && (uintptr_t)a < (uintptr_t)b + lb && (uintptr_t)b < (uintptr_t)a + la;
  };
  for (const StepOperand* w = operands.begin(); w != operands.end(); ++w) {
    if (!w->written) continue;
    for (const StepOperand* v = operands.begin(); v != operands.end(); ++v) {
      if (v == w || (v->written && v < w)) continue;   // (two written spans: seen from the earlier one)
      const bool partner = w->same == v - operands.begin();
      if (!(partner && w->p == v->p) && overlap(w->p, bytes * w->planes, v->p, bytes * v->planes))
        return refuse(partner ? "%s: %s may be %s itself, but must not overlap it in any other way" : "%s: %s must not overlap %s",
                      w->name, v->name);
    }
    if (coef.overlaps && overlap(w->p, bytes * w->planes, coef.p, coef.floats * sizeof(float)))
      return refuse("%s: %s must not overlap %s", w->name, "coef");
  }
  return finish(launch(rescale ? guidance_rescale : 0.0f), who);
}

// The argument rule of the InstructPix2Pix entries (ip2p.hip), stated once: an entry names its pointers in the header's order with the
// floats each spans -- paddlemix_amd/ip2p_forms.py holds the same rows for the Python side, tests/test_ip2p_host.py generates every
// refusal from them. A pointer that takes no part in the call (`used` false) is neither checked nor dereferenced. The rule: no null
// among the used pointers unless optional; the entry's own range check, after which the span lengths are meaningful; a written span
// overlaps no other used span.
struct Span {
  const char* name;
  const void* p;
  int64_t floats;
  bool written, optional, used;
};
template <class Launch>
static int span_entry(const char* who, std::initializer_list<Span> spans, const char* range_rule, bool in_range, Launch launch) {
  auto refuse = [who](const char* rule, const char* a = "", const char* b = "") {
    snprintf(g_err, sizeof(g_err), rule, who, a, b);
    return (int)SD_ERR_INVALID;
  };
  for (const Span& s : spans)
    if (s.used && !s.p && !s.optional) return refuse("%s: null pointer (%s)", s.name);
  if (!in_range) return refuse(range_rule);
  for (const Span& w : spans) {
    if (!w.written) continue;
    for (const Span& v : spans) {
      if (&v == &w || !v.used || !v.p) continue;
      const uintptr_t a = (uintptr_t)w.p, la = (uintptr_t)w.floats * 4, b = (uintptr_t)v.p, lb = (uintptr_t)v.floats * 4;
      if (a < b + lb && b < a + la) return refuse("%s: %s must not overlap %s", w.name, v.name);
    }
  }
  return finish(launch(), who);
}

// The view geometry both panorama entries (panorama.hip) share, as span_entry's range rule: the first rule the call breaks, with the
// argument's name in it ("%s" stands for the entry), or NULL. paddlemix_amd/panorama_forms.py geometry_rule states the same rules in
// the same order for the Python side. On success *window = batch * C * win_h * win_w, the floats of one view of the whole batch, and
// 4 * ny * nx * *window as well as 4 * batch * C * H * W fit int64_t.
static const char* view_rule(int batch, int C, int H, int W, int win_h, int win_w, int stride, int ny, int nx, int circular,
                             int64_t* window) {
  static thread_local char rule[160];
  const struct {
    const char* name;
    int v;
  } dims[] = {{"batch", batch}, {"C", C}, {"H", H}, {"W", W}, {"win_h", win_h}, {"win_w", win_w}, {"stride", stride}, {"ny", ny}, {"nx", nx}};
  for (const auto& d : dims)
    if (d.v < 1) {
      snprintf(rule, sizeof(rule), "%%s: %s must be >= 1", d.name);
      return rule;
    }
  if (win_h > H) return "%s: win_h is larger than H";
  if (win_w > W) return "%s: win_w is larger than W";
  if (((int64_t)ny - 1) * stride + win_h > H) return "%s: ny: the last row of views leaves the source ((ny - 1) * stride + win_h > H)";
  if (!circular && ((int64_t)nx - 1) * stride + win_w > W)
    return "%s: nx: the last column of views leaves the source ((nx - 1) * stride + win_w > W) without circular";
  if (circular && ((int64_t)nx - 1) * stride >= W) return "%s: nx: a circular view starts past the source ((nx - 1) * stride >= W)";
  int64_t src = 4, win = 4;
  for (int v : {batch, C, H, W})
    if (__builtin_mul_overflow(src, (int64_t)v, &src)) return "%s: H, W: the source's size in bytes is past int64_t";
  for (int v : {batch, C, win_h, win_w, ny, nx})
    if (__builtin_mul_overflow(win, (int64_t)v, &win)) return "%s: ny, nx: the views' size in bytes is past int64_t";
  *window = (int64_t)batch * C * win_h * win_w;
  return nullptr;
}

extern "C" {

int mi355x_sd_abi_version(void) { return MI355X_SD_ABI_VERSION; }

int mi355x_sd_elem_dtype(void) {
#ifdef MI355X_SD_F16
  return MI355X_SD_ELEM_F16;
#else
  return MI355X_SD_ELEM_BF16;
#endif
}

const char* mi355x_sd_last_error(void) { return g_err; }

int mi355x_sd_init(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SD_ERR_HIP, "mi355x_sd_init: no HIP device visible");
  if (device < 0 || device >= n) return fail(SD_ERR_INVALID, "mi355x_sd_init: device index out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(SD_ERR_HIP, "mi355x_sd_init: hipSetDevice failed");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(SD_ERR_HIP, "mi355x_sd_init: no properties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_init: device is %s, this library is built for gfx950 only",
                prop.gcnArchName);
  return SD_OK;
}

int mi355x_sd_linear(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K, const float* bias,
                     const float* rowbias, int rows_per_batch, int ld_rowbias, const void* R, int ldr, float out_scale,
                     int flags, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !W || !C) return fail(SD_ERR_INVALID, "mi355x_sd_linear: null pointer");
  if (int rc = check_ws(ws, ws_bytes, "mi355x_sd_linear")) return rc;
  GemmArgs g = gemm_args(A, lda, W, C, ldc, M, N, K, ws, ws_bytes);
  g.bias = bias; g.rowbias = rowbias; g.rows_per_batch = rows_per_batch; g.ld_rowbias = ld_rowbias;
  g.R = (const bf16*)R; g.ldr = ldr; g.out_scale = out_scale;
  epilogue_flags(g, flags, EPILOGUE_LINEAR);
  return finish(launch_gemm(g, S(stream)), "mi355x_sd_linear");
}

int mi355x_sd_linear_ex(const void* A, int lda, int a_rows_per_batch, int64_t a_batch_stride, const void* W,
                        const float* w_scale, void* C,
                        int ldc, int c_rows_per_batch, int64_t c_batch_stride, int M, int N, int K, const float* bias,
                        const float* rowbias, int ld_rowbias, const float* gate, int ld_gate, int rows_per_batch,
                        const void* R, int ldr, float out_scale, int flags, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !W || !C) return fail(SD_ERR_INVALID, "mi355x_sd_linear_ex: null pointer");
  if (int rc = check_ws(ws, ws_bytes, "mi355x_sd_linear_ex")) return rc;
  GemmArgs g = gemm_args(A, lda, W, C, ldc, M, N, K, ws, ws_bytes);
  g.a_rpb = a_rows_per_batch; g.a_bstride = (long)a_batch_stride;
  g.c_rpb = c_rows_per_batch; g.c_bstride = (long)c_batch_stride;
  g.bias = bias; g.rowbias = rowbias; g.rows_per_batch = rows_per_batch; g.ld_rowbias = ld_rowbias;
  g.gate = gate; g.ld_gate = ld_gate;
  g.wscale = w_scale;
  g.R = (const bf16*)R; g.ldr = ldr; g.out_scale = out_scale;
  epilogue_flags(g, flags, EPILOGUE_ALL);
  return finish(launch_gemm(g, S(stream)), "mi355x_sd_linear_ex");
}

int mi355x_sd_row_stats(const void* x, int rows, int C, int ldx, float eps, float* stats, void* stream) {
  if (!x || !stats) return fail(SD_ERR_INVALID, "mi355x_sd_row_stats: null pointer");
  return finish(launch_row_stats((const bf16*)x, rows, C, ldx, eps, stats, S(stream)), "mi355x_sd_row_stats");
}

int mi355x_sd_linear_ln(const void* A, int lda, const float* row_stats, const void* W, const float* w_rowsum, void* C,
                        int ldc, int M, int N, int K, const float* bias, int flags, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !W || !C || !row_stats || !w_rowsum) return fail(SD_ERR_INVALID, "mi355x_sd_linear_ln: null pointer");
  if (int rc = check_ws(ws, ws_bytes, "mi355x_sd_linear_ln")) return rc;
  GemmArgs g = gemm_args(A, lda, W, C, ldc, M, N, K, ws, ws_bytes);
  g.rowstat = row_stats; g.wsum = w_rowsum;
  g.bias = bias; g.out_scale = 1.0f;
  epilogue_flags(g, flags, EPILOGUE_ALL);
  return finish(launch_gemm(g, S(stream)), "mi355x_sd_linear_ln");
}

int mi355x_sd_linear_f8(const void* A8, int lda, int a_rows_per_batch, int64_t a_batch_stride, const float* a_scale,
                        const void* W8, const float* w_scale, void* C, int ldc, int c_rows_per_batch,
                        int64_t c_batch_stride, int M, int N, int K, const float* bias, const float* gate, int ld_gate,
                        int rows_per_batch, const void* R, int ldr, int flags, void* stream) {
  if (!A8 || !W8 || !C || !a_scale || !w_scale) return fail(SD_ERR_INVALID, "mi355x_sd_linear_f8: null pointer");
  if (flags & ~MI355X_SD_GELU_TANH) return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_linear_f8: only MI355X_SD_GELU_TANH is supported");
  GemmArgs g = gemm_args(A8, lda, W8, C, ldc, M, N, K);
  g.a_rpb = a_rows_per_batch; g.a_bstride = (long)a_batch_stride;
  g.c_rpb = c_rows_per_batch; g.c_bstride = (long)c_batch_stride;
  g.ascale = a_scale; g.wscale = w_scale;
  g.bias = bias; g.gate = gate; g.ld_gate = ld_gate; g.rows_per_batch = rows_per_batch;
  g.R = (const bf16*)R; g.ldr = ldr; g.out_scale = 1.0f;
  epilogue_flags(g, flags, MI355X_SD_GELU_TANH);
  return finish(launch_gemm_f8(g, S(stream)), "mi355x_sd_linear_f8");
}

int mi355x_sd_adaln_f8(const void* x, int rows, int C, int ldx, const float* scale, const float* shift, int ld_mod,
                       int rows_per_batch, float eps, void* y8, int ldy, float* y_scale, float* y_l2, void* stream) {
  if (!x || !scale || !shift || !y8 || !y_scale) return fail(SD_ERR_INVALID, "mi355x_sd_adaln_f8: null pointer");
  return finish(launch_adaln_f8((const bf16*)x, rows, C, ldx, scale, shift, ld_mod, rows_per_batch, eps, (unsigned char*)y8,
                                ldy, y_scale, y_l2, S(stream)), "mi355x_sd_adaln_f8");
}

int mi355x_sd_linear_f8_q(const void* A8, int lda, const float* a_scale, const float* a_l2, const void* W8,
                          const float* w_scale, float w_norm_max, void* C8, int ldc, float* c_scale, int M, int N, int K,
                          const float* bias, float bias_abs_max, int flags, void* stream) {
  if (!A8 || !W8 || !C8 || !a_scale || !a_l2 || !w_scale || !c_scale)
    return fail(SD_ERR_INVALID, "mi355x_sd_linear_f8_q: null pointer");
  if (flags & ~MI355X_SD_GELU_TANH) return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_linear_f8_q: only MI355X_SD_GELU_TANH is supported");
  GemmArgs g = gemm_args(A8, lda, W8, C8, ldc, M, N, K);
  g.ascale = a_scale; g.wscale = w_scale; g.bias = bias; g.out_scale = 1.0f;
  g.out_f8 = 1; g.a_l2 = a_l2; g.w_norm_max = w_norm_max; g.bias_abs_max = bias_abs_max; g.oscale = c_scale;
  epilogue_flags(g, flags, MI355X_SD_GELU_TANH);
  return finish(launch_gemm_f8(g, S(stream)), "mi355x_sd_linear_f8_q");
}

int mi355x_sd_quantize_rows(const void* x, int64_t rows, int C, int ldx, int x_rows_per_batch, int64_t x_batch_stride,
                            void* y8, int ldy, float* y_scale, void* stream) {
  if (!x || !y8 || !y_scale) return fail(SD_ERR_INVALID, "mi355x_sd_quantize_rows: null pointer");
  return finish(launch_quantize_rows((const bf16*)x, (long)rows, C, ldx, x_rows_per_batch, (long)x_batch_stride,
                                     (unsigned char*)y8, ldy, y_scale, S(stream)), "mi355x_sd_quantize_rows");
}

// ---- A base entry and its `_ex` form are one body (`*_entry`, which reports under the name of the entry that was called): the base
// entry is that body with the neutral value of the argument the `_ex` form adds. ----
static int adaln_entry(const char* who, const void* x, int rows, int C, int ldx, const void* scale, const void* shift, int ld_mod,
                       int mod_dtype, int rows_per_batch, float eps, void* y, int ldy, void* stream) {
  if (!x || !scale || !shift || !y) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  if (mod_dtype != MI355X_SD_MOD_F32 && mod_dtype != MI355X_SD_MOD_ELEM)
    return fail(SD_ERR_INVALID, "%s: mod_dtype must be MI355X_SD_MOD_F32 or MI355X_SD_MOD_ELEM", who);
  return finish(launch_adaln((const bf16*)x, rows, C, ldx, scale, shift, ld_mod, mod_dtype == MI355X_SD_MOD_ELEM, rows_per_batch, eps,
                             (bf16*)y, ldy, S(stream)), who);
}

int mi355x_sd_adaln(const void* x, int rows, int C, int ldx, const float* scale, const float* shift, int ld_mod,
                    int rows_per_batch, float eps, void* y, int ldy, void* stream) {
  return adaln_entry("mi355x_sd_adaln", x, rows, C, ldx, scale, shift, ld_mod, MI355X_SD_MOD_F32, rows_per_batch, eps, y, ldy, stream);
}

int mi355x_sd_adaln_ex(const void* x, int rows, int C, int ldx, const void* scale, const void* shift, int ld_mod, int mod_dtype,
                       int rows_per_batch, float eps, void* y, int ldy, void* stream) {
  return adaln_entry("mi355x_sd_adaln_ex", x, rows, C, ldx, scale, shift, ld_mod, mod_dtype, rows_per_batch, eps, y, ldy, stream);
}

int mi355x_sd_patchify(const float* x_nchw, int B, int C, int H, int W, int patch, void* out, int ldo, void* stream) {
  if (!x_nchw || !out) return fail(SD_ERR_INVALID, "mi355x_sd_patchify: null pointer");
  return finish(launch_patchify(x_nchw, B, C, H, W, patch, (bf16*)out, ldo, S(stream)), "mi355x_sd_patchify");
}

int mi355x_sd_unpatchify(const void* x, int ldx, int B, int C, int H, int W, int patch, float* out_nchw, void* stream) {
  if (!x || !out_nchw) return fail(SD_ERR_INVALID, "mi355x_sd_unpatchify: null pointer");
  return finish(launch_unpatchify((const bf16*)x, ldx, B, C, H, W, patch, out_nchw, S(stream)), "mi355x_sd_unpatchify");
}

int mi355x_sd_conv3x3(const void* X, int ldx, int B, int Hs, int Ws, int Cin, int stride, int upsample, const void* W,
                      void* C, int ldc, int Cout, const float* bias, const float* rowbias, int ld_rowbias,
                      const void* R, int ldr, float out_scale, int flags, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !W || !C) return fail(SD_ERR_INVALID, "mi355x_sd_conv3x3: null pointer");
  if (int rc = check_ws(ws, ws_bytes, "mi355x_sd_conv3x3")) return rc;
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2) ||
      (upsample != 0 && upsample != 1))
    return fail(SD_ERR_INVALID, "mi355x_sd_conv3x3: bad shape");
  if (flags & MI355X_SD_GEGLU) return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_conv3x3: GEGLU epilogue is linear-only");
  const int pad = (flags & MI355X_SD_PAD_BR) ? 0 : 1, kb64 = (flags & MI355X_SD_CONV_KB64) ? 1 : 0;
  if (kb64 && (Cin & 63)) return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_conv3x3: MI355X_SD_CONV_KB64 needs Cin % 64 == 0");
  if (!pad && (stride != 2 || upsample))
    return fail(SD_ERR_UNSUPPORTED, "mi355x_sd_conv3x3: MI355X_SD_PAD_BR is the stride-2 downsampler's padding");
  const int Hin = Hs << upsample, Win = Ws << upsample;
  // (bottom / right padding of a one-pixel row or column: the padded image is narrower than the window and has no output; C's
  // division truncates (1 + 1 - 3) / 2 to 0 and would compute one output row from a window that does not fit)
  if (!pad && (Hin < 2 || Win < 2)) return fail(SD_ERR_INVALID, "mi355x_sd_conv3x3: image smaller than the padded 3 x 3 window");
  const int Ho = (Hin + 1 + pad - 3) / stride + 1, Wo = (Win + 1 + pad - 3) / stride + 1;
  GemmArgs g = gemm_args(X, ldx, W, C, ldc, B * Ho * Wo, Cout, 9 * Cin, ws, ws_bytes);
  g.conv = 1; g.Hs = Hs; g.Ws = Ws; g.Ho = Ho; g.Wo = Wo; g.Cin = Cin; g.stride = stride; g.up = upsample; g.pad = pad; g.kb64 = kb64;
  g.bias = bias; g.rowbias = rowbias; g.rows_per_batch = Ho * Wo; g.ld_rowbias = ld_rowbias;
  g.R = (const bf16*)R; g.ldr = ldr; g.out_scale = out_scale;
  epilogue_flags(g, flags, EPILOGUE_CONV);
  return finish(launch_gemm(g, S(stream)), "mi355x_sd_conv3x3");
}

// The three attention entries are one body: `flags` are mi355x_sd_sdpa_ex's, `accum` is mi355x_sd_sdpa_accum's out_scale (NULL: the
// output is written, not added to).
static int sdpa_entry(const char* who, const void* q, const void* k, const void* v, const float* bias, void* out, int B, int H, int Sq,
                      int Skv, int D, int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts, int64_t o_bs, int o_ts,
                      int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale, int flags, const float* accum, void* stream) {
  if (!q || !k || !v || !out) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  if ((flags & MI355X_SD_SDPA_LOG2) && (bias || D != 64))
    return fail(SD_ERR_UNSUPPORTED, "%s: MI355X_SD_SDPA_LOG2 needs D == 64 and no mask", who);
  if (accum && *accum == 0.f) return SD_OK;   // out += 0 * attention
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = (const bf16*)q; a.K = (const bf16*)k; a.V = (const bf16*)v; a.O = (bf16*)out;
  a.B = B; a.H = H; a.Sq = Sq; a.Skv = Skv; a.D = D;
  a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs;
  a.q_ts = q_ts; a.k_ts = k_ts; a.v_ts = v_ts; a.o_ts = o_ts;
  a.bias = bias; a.bias_bs = bias_bs; a.bias_hs = bias_hs; a.bias_qs = bias_qs;
  a.log2 = (flags & MI355X_SD_SDPA_LOG2) ? 1 : 0;
  a.scale = a.log2 ? 1.0f : scale;
  a.accum = accum ? *accum : 0.f;
  return finish(launch_attention(a, S(stream)), who);
}

int mi355x_sd_sdpa(const void* q, const void* k, const void* v, const float* bias, void* out, int B, int H, int Sq,
                   int Skv, int D, int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts,
                   int64_t o_bs, int o_ts, int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale,
                   void* stream) {
  return sdpa_entry("mi355x_sd_sdpa", q, k, v, bias, out, B, H, Sq, Skv, D, q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts, bias_bs,
                    bias_hs, bias_qs, scale, 0, nullptr, stream);
}

int mi355x_sd_sdpa_ex(const void* q, const void* k, const void* v, const float* bias, void* out, int B, int H, int Sq,
                      int Skv, int D, int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts,
                      int64_t o_bs, int o_ts, int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale, int flags,
                      void* stream) {
  return sdpa_entry("mi355x_sd_sdpa_ex", q, k, v, bias, out, B, H, Sq, Skv, D, q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts, bias_bs,
                    bias_hs, bias_qs, scale, flags, nullptr, stream);
}

int mi355x_sd_sdpa_accum(const void* q, const void* k, const void* v, const float* bias, void* out, int B, int H, int Sq,
                         int Skv, int D, int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts,
                         int64_t o_bs, int o_ts, int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale,
                         float out_scale, void* stream) {
  return sdpa_entry("mi355x_sd_sdpa_accum", q, k, v, bias, out, B, H, Sq, Skv, D, q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts,
                    bias_bs, bias_hs, bias_qs, scale, 0, &out_scale, stream);
}

int mi355x_sd_groupnorm_workspace_floats(int B, int HW, int C) { return groupnorm_partial_floats(B, HW, C); }

static int groupnorm_stats_entry(const char* who, const void* x, int B, int HW, int C, int ldx, int groups, float eps, const float* gamma,
                                 const float* beta, float* workspace, float* scale_shift, int x_f32, void* stream) {
  if (!x || !gamma || !beta || !workspace || !scale_shift) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  return finish(launch_groupnorm_stats(x, x_f32, B, HW, C, ldx, groups, eps, gamma, beta, workspace, scale_shift, S(stream)), who);
}

int mi355x_sd_groupnorm_stats(const void* x, int B, int HW, int C, int ldx, int groups, float eps, const float* gamma,
                              const float* beta, float* workspace, float* scale_shift, void* stream) {
  return groupnorm_stats_entry("mi355x_sd_groupnorm_stats", x, B, HW, C, ldx, groups, eps, gamma, beta, workspace, scale_shift, 0, stream);
}

int mi355x_sd_groupnorm_stats_ex(const void* x, int B, int HW, int C, int ldx, int groups, float eps, const float* gamma,
                                 const float* beta, float* workspace, float* scale_shift, int x_f32, void* stream) {
  return groupnorm_stats_entry("mi355x_sd_groupnorm_stats_ex", x, B, HW, C, ldx, groups, eps, gamma, beta, workspace, scale_shift, x_f32,
                               stream);
}

int mi355x_sd_groupnorm_act_fits(int HW, int C, int groups) { return groupnorm_act_fits(HW, C, groups); }

int mi355x_sd_groupnorm_act(const void* x, int B, int HW, int C, int ldx, int groups, float eps, const float* gamma, const float* beta,
                            int silu, void* y, int ldy, void* stream) {
  if (!x || !gamma || !beta || !y) return fail(SD_ERR_INVALID, "mi355x_sd_groupnorm_act: null pointer");
  return finish(launch_groupnorm_act((const bf16*)x, B, HW, C, ldx, groups, eps, gamma, beta, silu, (bf16*)y, ldy, S(stream)),
                "mi355x_sd_groupnorm_act");
}

static int scale_shift_act_entry(const char* who, const void* x, int B, int HW, int C, int ldx, const float* scale_shift, int silu, void* y,
                                 int ldy, int x_f32, void* raw16, int ld_raw, void* stream) {
  if (!x || !scale_shift || !y) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  return finish(launch_scale_shift_act(x, x_f32, B, HW, C, ldx, scale_shift, silu, (bf16*)y, ldy, (bf16*)raw16, ld_raw, S(stream)), who);
}

int mi355x_sd_scale_shift_act(const void* x, int B, int HW, int C, int ldx, const float* scale_shift, int silu, void* y,
                              int ldy, void* stream) {
  return scale_shift_act_entry("mi355x_sd_scale_shift_act", x, B, HW, C, ldx, scale_shift, silu, y, ldy, 0, nullptr, 0, stream);
}

int mi355x_sd_scale_shift_act_ex(const void* x, int B, int HW, int C, int ldx, const float* scale_shift, int silu, void* y,
                                 int ldy, int x_f32, void* raw16, int ld_raw, void* stream) {
  return scale_shift_act_entry("mi355x_sd_scale_shift_act_ex", x, B, HW, C, ldx, scale_shift, silu, y, ldy, x_f32, raw16, ld_raw, stream);
}

static int layernorm_entry(const char* who, const void* x, int rows, int C, int ldx, const float* gamma, const float* beta, float eps,
                           void* y, int ldy, int x_f32, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  return finish(launch_layernorm(x, x_f32, rows, C, ldx, gamma, beta, eps, (bf16*)y, ldy, S(stream)), who);
}

int mi355x_sd_layernorm(const void* x, int rows, int C, int ldx, const float* gamma, const float* beta, float eps,
                        void* y, int ldy, void* stream) {
  return layernorm_entry("mi355x_sd_layernorm", x, rows, C, ldx, gamma, beta, eps, y, ldy, 0, stream);
}

int mi355x_sd_layernorm_ex(const void* x, int rows, int C, int ldx, const float* gamma, const float* beta, float eps,
                           void* y, int ldy, int x_f32, void* stream) {
  return layernorm_entry("mi355x_sd_layernorm_ex", x, rows, C, ldx, gamma, beta, eps, y, ldy, x_f32, stream);
}

static int fused_adaln_scale_residual_entry(const char* who, const void* x, int ldx, const void* mha_out, int ld_mha, const void* gate_msa,
                                            const void* scale_mlp, const void* shift_mlp, int ld_mod, int mod_dtype,
                                            int rows_per_batch, const void* weight, const void* bias, float epsilon, int rows, int C,
                                            void* resi_out, int ld_resi, void* adaln_out, int ld_out, void* stream) {
  if (!x || !mha_out || !gate_msa || !scale_mlp || !shift_mlp || !resi_out || !adaln_out)
    return fail(SD_ERR_INVALID, "%s: null pointer", who);
  if (mod_dtype != MI355X_SD_MOD_F32 && mod_dtype != MI355X_SD_MOD_ELEM)
    return fail(SD_ERR_INVALID, "%s: mod_dtype must be MI355X_SD_MOD_F32 or MI355X_SD_MOD_ELEM", who);
  return finish(launch_fused_adaln_scale_residual((const bf16*)x, ldx, (const bf16*)mha_out, ld_mha, gate_msa, scale_mlp, shift_mlp,
                                                  ld_mod, mod_dtype == MI355X_SD_MOD_ELEM, rows_per_batch, weight, bias, epsilon, rows,
                                                  C, (bf16*)resi_out, ld_resi, (bf16*)adaln_out, ld_out, S(stream)), who);
}

int mi355x_sd_fused_adaln_scale_residual(const void* x, int ldx, const void* mha_out, int ld_mha, const float* gate_msa,
                                         const float* scale_mlp, const float* shift_mlp, int ld_mod, int rows_per_batch,
                                         const float* weight, const float* bias, float epsilon, int rows, int C, void* resi_out,
                                         int ld_resi, void* adaln_out, int ld_out, void* stream) {
  return fused_adaln_scale_residual_entry("mi355x_sd_fused_adaln_scale_residual", x, ldx, mha_out, ld_mha, gate_msa, scale_mlp, shift_mlp,
                                          ld_mod, MI355X_SD_MOD_F32, rows_per_batch, weight, bias, epsilon, rows, C, resi_out, ld_resi,
                                          adaln_out, ld_out, stream);
}

int mi355x_sd_fused_adaln_scale_residual_ex(const void* x, int ldx, const void* mha_out, int ld_mha, const void* gate_msa,
                                            const void* scale_mlp, const void* shift_mlp, int ld_mod, int mod_dtype,
                                            int rows_per_batch, const void* weight, const void* bias, float epsilon, int rows, int C,
                                            void* resi_out, int ld_resi, void* adaln_out, int ld_out, void* stream) {
  return fused_adaln_scale_residual_entry("mi355x_sd_fused_adaln_scale_residual_ex", x, ldx, mha_out, ld_mha, gate_msa, scale_mlp,
                                          shift_mlp, ld_mod, mod_dtype, rows_per_batch, weight, bias, epsilon, rows, C, resi_out, ld_resi,
                                          adaln_out, ld_out, stream);
}

int mi355x_sd_split_concat(const void* x, const void* y, void* q_out, void* k_out, void* v_out, int B, int S1, int S2, int C,
                           void* stream) {
  if (!x || !y || !q_out || !k_out || !v_out) return fail(SD_ERR_INVALID, "mi355x_sd_split_concat: null pointer");
  return finish(launch_split_concat((const bf16*)x, (const bf16*)y, (bf16*)q_out, (bf16*)k_out, (bf16*)v_out, B, S1, S2, C, S(stream)),
                "mi355x_sd_split_concat");
}

int mi355x_sd_timestep_embedding(const float* t, int t_count, int n, int dim, int group, int flip_sin_to_cos,
                                 float freq_shift, float scale, float max_period, void* out, int ldo, void* stream) {
  if (!t || !out) return fail(SD_ERR_INVALID, "mi355x_sd_timestep_embedding: null pointer");
  return finish(launch_timestep_embedding(t, t_count, n, dim, group, flip_sin_to_cos, freq_shift, scale, max_period,
                                          (bf16*)out, ldo, S(stream)),
                "mi355x_sd_timestep_embedding");
}

int mi355x_sd_silu(const void* x, void* y, int64_t n, int in_f32, int out_f32, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_silu: null pointer");
  return finish(launch_silu(x, y, (long)n, in_f32, out_f32, S(stream)), "mi355x_sd_silu");
}

static int conv_in3x3_entry(const char* who, const float* x_nchw, const float* in_scale, const void* w, const float* bias, void* y, int B,
                            int Cin, int H, int W, int Cout, int ldy, int out_f32, void* stream) {
  if (!x_nchw || !w || !y) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  return finish(launch_conv_in3x3(x_nchw, in_scale, (const bf16*)w, bias, y, out_f32, B, Cin, H, W, Cout, ldy, S(stream)), who);
}

int mi355x_sd_conv_in3x3(const float* x_nchw, const float* in_scale, const void* w, const float* bias, void* y, int B,
                         int Cin, int H, int W, int Cout, int ldy, void* stream) {
  return conv_in3x3_entry("mi355x_sd_conv_in3x3", x_nchw, in_scale, w, bias, y, B, Cin, H, W, Cout, ldy, 0, stream);
}

int mi355x_sd_conv_in3x3_ex(const float* x_nchw, const float* in_scale, const void* w, const float* bias, void* y, int B,
                            int Cin, int H, int W, int Cout, int ldy, int out_f32, void* stream) {
  return conv_in3x3_entry("mi355x_sd_conv_in3x3_ex", x_nchw, in_scale, w, bias, y, B, Cin, H, W, Cout, ldy, out_f32, stream);
}

int mi355x_sd_cast_rows(const float* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_cast_rows: null pointer");
  return finish(launch_cast_rows(x, ldx, (bf16*)y, ldy, (long)rows, C, S(stream)), "mi355x_sd_cast_rows");
}

int mi355x_sd_conv_out3x3(const void* x, int ldx, const void* w, const float* bias, float* y_nchw, int B, int Cin, int H,
                          int W, int Cout, void* stream) {
  if (!x || !w || !y_nchw) return fail(SD_ERR_INVALID, "mi355x_sd_conv_out3x3: null pointer");
  return finish(launch_conv_out3x3((const bf16*)x, ldx, (const bf16*)w, bias, y_nchw, B, Cin, H, W, Cout, S(stream)),
                "mi355x_sd_conv_out3x3");
}

int mi355x_sd_copy_rows(const void* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_copy_rows: null pointer");
  return finish(launch_copy_rows((const bf16*)x, ldx, (bf16*)y, ldy, (long)rows, C, S(stream)), "mi355x_sd_copy_rows");
}

static int add_nchw_entry(const char* who, void* x, int ldx, const float* r_nchw, int B, int C, int64_t HW, int x_f32, void* stream) {
  if (!x || !r_nchw) return fail(SD_ERR_INVALID, "%s: null pointer", who);
  return finish(launch_add_nchw(x, x_f32, ldx, r_nchw, B, C, (long)HW, S(stream)), who);
}

int mi355x_sd_add_nchw(void* x, int ldx, const float* r_nchw, int B, int C, int64_t HW, void* stream) {
  return add_nchw_entry("mi355x_sd_add_nchw", x, ldx, r_nchw, B, C, HW, 0, stream);
}

int mi355x_sd_add_nchw_ex(void* x, int ldx, const float* r_nchw, int B, int C, int64_t HW, int x_f32, void* stream) {
  return add_nchw_entry("mi355x_sd_add_nchw_ex", x, ldx, r_nchw, B, C, HW, x_f32, stream);
}

int mi355x_sd_latent_dist(const float* moments, int ld, int B, int L, int64_t HW, const float* noise_nchw, float out_scale,
                          float* mean_nchw, float* logvar_nchw, float* sample_nchw, void* stream) {
  if (!moments || !mean_nchw || !logvar_nchw) return fail(SD_ERR_INVALID, "mi355x_sd_latent_dist: null pointer");
  return finish(launch_latent_dist(moments, ld, B, L, (long)HW, noise_nchw, out_scale, mean_nchw, logvar_nchw, sample_nchw,
                                   S(stream)), "mi355x_sd_latent_dist");
}

int mi355x_sd_embed_tokens(const int32_t* ids, int64_t n_tokens, int seq_len, const void* token_table,
                           const void* position_table, int D, void* out, int ldo, void* stream) {
  if (!ids || !token_table || !out) return fail(SD_ERR_INVALID, "mi355x_sd_embed_tokens: null pointer");
  return finish(launch_embed_tokens(ids, (long)n_tokens, seq_len, (const bf16*)token_table, (const bf16*)position_table, D,
                                    (bf16*)out, ldo, S(stream)), "mi355x_sd_embed_tokens");
}

int mi355x_sd_rmsnorm(const void* x, int rows, int C, int ldx, const float* weight, float eps, void* y, int ldy,
                      void* stream) {
  if (!x || !weight || !y) return fail(SD_ERR_INVALID, "mi355x_sd_rmsnorm: null pointer");
  return finish(launch_rmsnorm((const bf16*)x, rows, C, ldx, weight, eps, (bf16*)y, ldy, S(stream)), "mi355x_sd_rmsnorm");
}

int mi355x_sd_gated_activation(const void* x, int ldx, void* y, int ldy, int64_t rows, int F, int kind, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_gated_activation: null pointer");
  return finish(launch_gated_activation((const bf16*)x, ldx, (bf16*)y, ldy, (long)rows, F, kind, S(stream)),
                "mi355x_sd_gated_activation");
}

int mi355x_sd_activation(const void* x, void* y, int64_t n, int kind, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_activation: null pointer");
  return finish(launch_activation((const bf16*)x, (bf16*)y, (long)n, kind, S(stream)), "mi355x_sd_activation");
}

int mi355x_sd_conv1x1_nchw(const float* x_nchw, float in_scale, const void* w, const float* bias, float* y_nchw, int B,
                           int Cin, int Cout, int64_t HW, void* stream) {
  if (!x_nchw || !w || !y_nchw) return fail(SD_ERR_INVALID, "mi355x_sd_conv1x1_nchw: null pointer");
  return finish(launch_conv1x1_nchw(x_nchw, in_scale, (const bf16*)w, bias, y_nchw, B, Cin, Cout, (long)HW, S(stream)),
                "mi355x_sd_conv1x1_nchw");
}

int mi355x_sd_tile_gather(const float* src_nchw, int B, int C, int H, int W, int y0, int x0, int stride_y, int stride_x, int ny,
                          int nx, int win_h, int win_w, int64_t first, int64_t count, float* dst, void* stream) {
  if (!src_nchw || !dst) return fail(SD_ERR_INVALID, "mi355x_sd_tile_gather: null pointer");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ny <= 0 || nx <= 0 || win_h <= 0 || win_w <= 0)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_gather: sizes and grid counts must be positive");
  if (y0 < 0 || x0 < 0 || stride_y < 0 || stride_x < 0 || (int64_t)y0 + (int64_t)(ny - 1) * stride_y + win_h > H ||
      (int64_t)x0 + (int64_t)(nx - 1) * stride_x + win_w > W)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_gather: a window of the grid leaves the source tensor");
  if (first < 0 || count <= 0 || first + count > (int64_t)B * ny * nx)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_gather: [first, first + count) is not a range of the B * ny * nx windows");
  return finish(launch_tile_gather(src_nchw, B, C, H, W, y0, x0, stride_y, stride_x, ny, nx, win_h, win_w, (long)first, (long)count,
                                   dst, S(stream)), "mi355x_sd_tile_gather");
}

int mi355x_sd_tile_blend(const void* tile_ptrs, int B, int C, int H, int W, int S_, int lim, int ext, int ny, int nx,
                         int64_t t_chan_plane, int64_t t_chan, int64_t t_col, float* out, int64_t o_img, int64_t o_chan, int64_t o_row,
                         int64_t o_col, void* stream) {
  if (!tile_ptrs || !out) return fail(SD_ERR_INVALID, "mi355x_sd_tile_blend: null pointer");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || S_ <= 0 || lim <= 0 || ext < 0)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_blend: sizes must be positive (ext >= 0)");
  if (ext > lim || lim > S_)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_blend: needs ext <= lim <= S (a blend must read outside the neighbour's own band)");
  if (ny != (H + lim - 1) / lim || nx != (W + lim - 1) / lim)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_blend: ny, nx must be ceil(H / lim), ceil(W / lim)");
  if (t_chan_plane < 0 || t_chan < 0 || t_col <= 0 || o_img < 0 || o_chan < 0 || o_row <= 0 || o_col <= 0)
    return fail(SD_ERR_INVALID, "mi355x_sd_tile_blend: strides must be positive");
  return finish(launch_tile_blend((const float* const*)tile_ptrs, B, C, H, W, S_, lim, ext, ny, nx, (long)t_chan_plane, (long)t_chan,
                                  (long)t_col, out, (long)o_img, (long)o_chan, (long)o_row, (long)o_col, S(stream)),
                "mi355x_sd_tile_blend");
}

int mi355x_sd_softmax_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int n, void* stream) {
  if (!x || !y) return fail(SD_ERR_INVALID, "mi355x_sd_softmax_rows: null pointer");
  return finish(launch_softmax_rows(x, (long)ldx, (bf16*)y, (long)ldy, (long)rows, n, S(stream)),
                "mi355x_sd_softmax_rows");
}

int mi355x_sd_axpby(const float* x, const float* y, float* out, const float* coef, int64_t n, void* stream) {
  if (!x || !y || !out || !coef) return fail(SD_ERR_INVALID, "mi355x_sd_axpby: null pointer");
  return finish(launch_axpby(x, y, out, coef, (long)n, S(stream)), "mi355x_sd_axpby");
}

int mi355x_sd_mask_to_bias(const float* mask, float* bias, int64_t n, void* stream) {
  if (!mask || !bias) return fail(SD_ERR_INVALID, "mi355x_sd_mask_to_bias: null pointer");
  return finish(launch_mask_to_bias(mask, bias, (long)n, S(stream)), "mi355x_sd_mask_to_bias");
}

int mi355x_sd_cfg_axpby(const float* x, const float* eps_uncond, const float* eps_text, float* out, const float* coef,
                        float guidance_scale, int64_t n, void* stream) {
  if (!x || !eps_uncond || !eps_text || !out || !coef) return fail(SD_ERR_INVALID, "mi355x_sd_cfg_axpby: null pointer");
  return finish(launch_cfg_axpby(x, eps_uncond, eps_text, out, coef, guidance_scale, (long)n, S(stream)), "mi355x_sd_cfg_axpby");
}

// ---- the step-tail entries (step_tail.hip): each is one call of step_entry(), defined before the extern "C" block ----
int mi355x_sd_cfg_rescale_axpby(const float* x, const float* eps_uncond, const float* eps_text, float* out, const float* coef,
                                float guidance_scale, float guidance_rescale, int batch, int64_t per_sample, void* stream) {
  return step_entry("mi355x_sd_cfg_rescale_axpby", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text),
                                                    writes("out", out, 1, 0)},
                    {coef, 2, 1, false}, eps_text, guidance_rescale, true, batch, per_sample, [&](float gr) {
                      return launch_cfg_rescale_axpby(x, eps_uncond, eps_text, out, coef, guidance_scale, gr, batch, (long)per_sample,
                                                      S(stream));
                    });
}

int mi355x_sd_multistep_update(const float* x, const float* eps_uncond, const float* eps_text, const float* m_prev, float* out,
                               float* m_out, const float* coef, float guidance_scale, float guidance_rescale, int batch,
                               int64_t per_sample, void* stream) {
  return step_entry("mi355x_sd_multistep_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                                   reads("m_prev", m_prev), writes("out", out, 1, 0), writes("m_out", m_out, 1, 3)},
                    {coef, 5, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_multistep_update(x, eps_uncond, eps_text, m_prev, out, m_out, coef, guidance_scale, gr, batch,
                                                     (long)per_sample, S(stream));
                    });
}

int mi355x_sd_unipc_update(const float* x, const float* eps_uncond, const float* eps_text, float* last, float* hist, int order,
                           float* out, const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                           void* stream) {
  if (order < 1 || order > 3) return fail(SD_ERR_INVALID, "%s: order must be 1, 2 or 3 (the planes of hist)", "mi355x_sd_unipc_update");
  return step_entry("mi355x_sd_unipc_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                               writes("last", last), writes("hist", hist, order), writes("out", out, 1, 0)},
                    {coef, 12, 16, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_unipc_update(x, eps_uncond, eps_text, last, hist, order, out, coef, guidance_scale, gr, batch,
                                                 (long)per_sample, S(stream));
                    });
}

int mi355x_sd_ancestral_update(const float* x, const float* eps_uncond, const float* eps_text, const float* noise, float* out,
                               const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                               void* stream) {
  return step_entry("mi355x_sd_ancestral_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                                   reads("noise", noise, true), writes("out", out, 1, 0)},   // (noise: see the header)
                    {coef, 3, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_ancestral_update(x, eps_uncond, eps_text, noise, out, coef, guidance_scale, gr, batch,
                                                     (long)per_sample, S(stream));
                    });
}

int mi355x_sd_heun_update(const float* x, const float* eps_uncond, const float* eps_text, float* sample, float* deriv, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream) {
  return step_entry("mi355x_sd_heun_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                              writes("sample", sample), writes("deriv", deriv), writes("out", out, 1, 0)},
                    {coef, 5, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_heun_update(x, eps_uncond, eps_text, sample, deriv, out, coef, guidance_scale, gr, batch,
                                                (long)per_sample, S(stream));
                    });
}

int mi355x_sd_dpm2_update(const float* x, const float* eps_uncond, const float* eps_text, const float* noise, float* sample, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream) {
  return step_entry("mi355x_sd_dpm2_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                              reads("noise", noise, true), writes("sample", sample), writes("out", out, 1, 0)},
                    {coef, 5, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {   // (noise: see the header)
                      return launch_dpm2_update(x, eps_uncond, eps_text, noise, sample, out, coef, guidance_scale, gr, batch,
                                                (long)per_sample, S(stream));
                    });
}

int mi355x_sd_plms_update(const float* x, const float* eps_uncond, const float* eps_text, float* park, float* hist, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream) {
  return step_entry("mi355x_sd_plms_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                              writes("park", park), writes("hist", hist, 3), writes("out", out, 1, 0)},
                    {coef, 12, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_plms_update(x, eps_uncond, eps_text, park, hist, out, coef, guidance_scale, gr, batch,
                                                (long)per_sample, S(stream));
                    });
}

int mi355x_sd_singlestep_update(const float* x, const float* eps_uncond, const float* eps_text, float* park, float* hist, float* out,
                                const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                                void* stream) {
  return step_entry("mi355x_sd_singlestep_update", {reads("x", x), reads("eps_uncond", eps_uncond), reads("eps_text", eps_text, true),
                                                    writes("park", park), writes("hist", hist, 2), writes("out", out, 1, 0)},
                    {coef, 8, 1, true}, eps_text, guidance_rescale, false, batch, per_sample, [&](float gr) {
                      return launch_singlestep_update(x, eps_uncond, eps_text, park, hist, out, coef, guidance_scale, gr, batch,
                                                      (long)per_sample, S(stream));
                    });
}

// ---- the InstructPix2Pix entries (ip2p.hip): each is one call of span_entry(), defined before the extern "C" block ----
int mi355x_sd_guidance3(const float* eps, const float* x, const float* coef, float* out, float guidance_scale,
                        float image_guidance_scale, float guidance_rescale, int batch, int64_t per_sample, void* stream) {
  const bool rescale = guidance_rescale > 0.0f, x0 = rescale && x;
  const bool ok = batch > 0 && per_sample >= (rescale ? 2 : 1) && per_sample <= INT64_MAX / 4 / 3 / batch;
  const int64_t n = ok ? (int64_t)batch * per_sample : 0;
  return span_entry("mi355x_sd_guidance3", {{"eps", eps, 3 * n, false, false, true}, {"x", x, n, false, true, rescale},
                                            {"coef", coef, 1, false, false, x0}, {"out", out, n, true, false, true}},
                    "%s: needs batch > 0 and per_sample >= 1 (>= 2 with guidance_rescale: the estimator divides by per_sample - 1)", ok,
                    [&] {
                      return launch_guidance3(eps, x0 ? x : nullptr, x0 ? coef : nullptr, out, guidance_scale, image_guidance_scale,
                                              rescale ? guidance_rescale : 0.0f, batch, (long)per_sample, S(stream));
                    });
}

int mi355x_sd_ip2p_input(const float* x, const float* image_latents, float* out, float scale, int groups, int batch, int c_lat,
                         int c_img, int64_t hw, void* stream) {
  const bool ok = groups > 0 && batch > 0 && c_lat > 0 && c_img > 0 && hw > 0 &&
                  hw <= INT64_MAX / 4 / groups / batch / ((int64_t)c_lat + c_img);
  const int64_t gb = ok ? (int64_t)groups * batch : 0;
  return span_entry("mi355x_sd_ip2p_input", {{"x", x, ok ? (int64_t)batch * c_lat * hw : 0, false, false, true},
                                             {"image_latents", image_latents, gb * c_img * hw, false, false, true},
                                             {"out", out, gb * ((int64_t)c_lat + c_img) * hw, true, false, true}},
                    "%s: needs groups, batch, c_lat, c_img and hw >= 1", ok, [&] {
                      return launch_ip2p_input(x, image_latents, out, scale, groups, batch, c_lat, c_img, (long)hw, S(stream));
                    });
}

// ---- semantic guidance (sega.hip): the same span rule; paddlemix_amd/sega_forms.py holds the row for the Python side ----
int mi355x_sd_sega_guidance(const float* eps, float* momentum, const float* extra, const float* row, float* out, float* stats,
                            int n_concepts, int batch, int channels, int64_t hw, void* stream) {
  const bool ok = n_concepts > 0 && batch > 0 && channels > 0 && hw > 0 &&
                  hw <= INT64_MAX / 4 / ((int64_t)n_concepts + 2) / batch / channels;
  const int64_t planes = ok ? (int64_t)batch * channels : 0, n = planes * hw;
  return span_entry("mi355x_sd_sega_guidance",
                    {{"eps", eps, (2 + (int64_t)n_concepts) * n, false, false, true},
                     {"momentum", momentum, n, true, false, true},
                     {"extra", extra, n, false, true, extra != nullptr},
                     {"row", row, 8 + 5 * (int64_t)n_concepts, false, false, true},
                     {"out", out, n, true, false, true},
                     {"stats", stats, 3 * n_concepts * planes, true, true, stats != nullptr}},
                    "%s: needs n_concepts, batch, channels and hw >= 1", ok, [&] {
                      return launch_sega_guidance(eps, momentum, extra, row, out, stats, n_concepts, batch, channels, (long)hw, S(stream));
                    });
}

// ---- panorama / MultiDiffusion (panorama.hip): the same span rule, the range rule from view_rule() above; paddlemix_amd/
// panorama_forms.py holds the rows for the Python side ----
int mi355x_sd_view_input(const float* x, float* out, float scale, int groups, int batch, int C, int H, int W, int win_h, int win_w,
                         int stride, int ny, int nx, int circular, int first, int count, void* stream) {
  int64_t window = 0;
  const char* bad = (groups != 1 && groups != 2) ? "%s: groups must be 1 or 2"
                                                 : view_rule(batch, C, H, W, win_h, win_w, stride, ny, nx, circular, &window);
  if (!bad && (first < 0 || count < 0 || (int64_t)first + count > (int64_t)ny * nx))
    bad = "%s: first, count: [first, first + count) is not a range of the ny * nx views";
  if (!bad && count > 0 && count > INT64_MAX / 4 / groups / window) bad = "%s: count: out's size in bytes is past int64_t";
  return span_entry("mi355x_sd_view_input", {{"x", x, bad ? 0 : (int64_t)batch * C * H * W, false, false, true},
                                             {"out", out, bad ? 0 : groups * count * window, true, false, true}},
                    bad ? bad : "", !bad, [&] {
                      return launch_view_input(x, out, scale, groups, batch, C, H, W, win_h, win_w, stride, ny, nx, circular, first,
                                               count, S(stream));
                    });
}

int mi355x_sd_view_merge(const float* views, float* out, int batch, int C, int H, int W, int win_h, int win_w, int stride, int ny,
                         int nx, int circular, void* stream) {
  int64_t window = 0;
  const char* bad = view_rule(batch, C, H, W, win_h, win_w, stride, ny, nx, circular, &window);
  return span_entry("mi355x_sd_view_merge", {{"views", views, bad ? 0 : (int64_t)ny * nx * window, false, false, true},
                                             {"out", out, bad ? 0 : (int64_t)batch * C * H * W, true, false, true}},
                    bad ? bad : "", !bad, [&] {
                      return launch_view_merge(views, out, batch, C, H, W, win_h, win_w, stride, ny, nx, circular, S(stream));
                    });
}

int mi355x_sd_graph_begin(void* stream) {
  if (hipStreamBeginCapture(S(stream), hipStreamCaptureModeThreadLocal) != hipSuccess)
    return finish(SD_ERR_HIP, "mi355x_sd_graph_begin");
  return SD_OK;
}

int mi355x_sd_graph_end(void* stream, void** graph_exec) {
  if (!graph_exec) return fail(SD_ERR_INVALID, "mi355x_sd_graph_end: null pointer");
  hipGraph_t graph = nullptr;
  if (hipStreamEndCapture(S(stream), &graph) != hipSuccess || !graph) return finish(SD_ERR_HIP, "mi355x_sd_graph_end");
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) return finish(SD_ERR_HIP, "mi355x_sd_graph_end(instantiate)");
  *graph_exec = exec;
  return SD_OK;
}

int mi355x_sd_graph_launch(void* graph_exec, void* stream) {
  if (!graph_exec) return fail(SD_ERR_INVALID, "mi355x_sd_graph_launch: null graph");
  if (hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph_exec), S(stream)) != hipSuccess)
    return finish(SD_ERR_HIP, "mi355x_sd_graph_launch");
  return SD_OK;
}

int mi355x_sd_graph_destroy(void* graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(graph_exec));
  return SD_OK;
}

int mi355x_sd_probe_layouts(float* out, void* stream) {
  if (!out) return fail(SD_ERR_INVALID, "mi355x_sd_probe_layouts: null pointer");
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, S(stream), out);
  return finish(hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP, "mi355x_sd_probe_layouts");
}

}  // extern "C"
