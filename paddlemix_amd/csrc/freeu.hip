// FreeU (https://arxiv.org/abs/2309.11497; the reference's apply_freeu / fourier_filter, utils/paddle_utils.py:259-313) on a concat buffer
// of the U-Net's up path: rows [B * H * W][ld >= Cx + Cs], backbone columns first, skip columns after (unet.py skip_layout).
//
//   columns [0, Cx / 2)       *= b
//   columns [Cx, Cx + Cs)     <- fourier_filter(plane, threshold = 1, scale = s), per (batch, channel) plane
//
// The reference's filter scales the four shifted FFT bins ky, kx in {-1, 0} of a real plane by s. Written out, that is
//
//   out = x + (s - 1) (<x> + sum over phi in {ty, tx, ty + tx} of <x cos phi> cos phi + <x sin phi> sin phi),
//   ty = 2 pi y / H, tx = 2 pi x / W, <.> the mean over the plane:
//
// seven sums per plane and one elementwise pass, no FFT. Two launches:
//   freeu_stats_kernel  the seven sums of every skip plane. A thread owns one 16-byte group of adjacent channels and walks whole image
//                       rows: per pixel the three row sums (1, cos tx, sin tx), per row their seven products with (1, cos ty, sin ty) --
//                       cos / sin (ty + tx) by angle addition. The rows of a plane are split over blockIdx.y (freeu_rows_per_split) when
//                       batch x channels alone would not fill the chip; the partial sums of a block's row slots are added in slot order
//                       through LDS and stored to workspace[b][split][7][channels], no atomics: the same bits on every run.
//   freeu_apply_kernel  adds the splits in order, folds the seven means into three per-row coefficients E, F, G per channel
//                       (correction = E + cos tx F + sin tx G), and rewrites the skip columns; the blocks of the first grid columns
//                       scale the backbone half instead. One rounding per stored element.
// cos / sin of tx come from an LDS table built per block by sincospif of the exact rational 2 x / W (folded to [-1, 1]); those of ty are
// computed once per image row. Column groups are aligned to the row start, so Cx may be odd: a group that straddles a region boundary
// is handled element by element, every other one with 16-byte loads and stores.
#include <math.h>

#include "../../include/mi355x_sd.h"
#include "common.h"
#include "kernels.h"

namespace sd {
namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_TARGET_BLOCKS = 512; // two blocks per CU before the plane is split no further (at most FU_MAX_SPLIT times, kernels.h)
constexpr int FU_MAX_W = 4096;        // the LDS table of tx holds 2 W floats

// the 16-byte column groups [g0, g0 + ng) that cover columns [c0, c1), nc grid columns of gw groups each, ty row slots per block
struct FuCols {
  int g0, ng, nc, gw, ty;
};
FuCols freeu_cols(int c0, int c1, int vec) {
  FuCols f{0, 0, 0, 1, FU_THREADS};
  if (c1 <= c0) return f;
  f.g0 = c0 / vec;
  f.ng = (c1 + vec - 1) / vec - f.g0;
  f.nc = (f.ng + kWave - 1) / kWave;
  f.gw = (f.ng + f.nc - 1) / f.nc;
  f.ty = FU_THREADS / f.gw;
  return f;
}
// rows per split of a plane of H image rows: as many splits as it takes to reach FU_TARGET_BLOCKS blocks, every row slot of a block busy
int freeu_rows_per_split(int B, int H, const FuCols& f) {
  const long blocks = (long)B * (f.nc > 0 ? f.nc : 1);
  long want = (FU_TARGET_BLOCKS + blocks - 1) / blocks;
  const long most = (H + f.ty - 1) / f.ty;
  if (want > most) want = most;
  if (want > FU_MAX_SPLIT) want = FU_MAX_SPLIT;
  if (want < 1) want = 1;
  return (int)((H + want - 1) / want);
}

template <bool F32>
struct FuElem;
template <>
struct FuElem<true> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const void* p, size_t i, float (&v)[V]) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(static_cast<const float*>(p) + i);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = t[j];
  }
  static __device__ __forceinline__ void store(void* p, size_t i, const float (&v)[V]) {
    f32x4 t;
#pragma unroll
    for (int j = 0; j < V; ++j) t[j] = v[j];
    *reinterpret_cast<f32x4*>(static_cast<float*>(p) + i) = t;
  }
  static __device__ __forceinline__ float load1(const void* p, size_t i) { return static_cast<const float*>(p)[i]; }
  static __device__ __forceinline__ void store1(void* p, size_t i, float v) { static_cast<float*>(p)[i] = v; }
};
template <>
struct FuElem<false> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void load(const void* p, size_t i, float (&v)[V]) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(static_cast<const bf16*>(p) + i);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (float)t[j];
  }
  static __device__ __forceinline__ void store(void* p, size_t i, const float (&v)[V]) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < V; ++j) t[j] = (bf16)v[j];
    *reinterpret_cast<bf16x8*>(static_cast<bf16*>(p) + i) = t;
  }
  static __device__ __forceinline__ float load1(const void* p, size_t i) { return (float)static_cast<const bf16*>(p)[i]; }
  static __device__ __forceinline__ void store1(void* p, size_t i, float v) { static_cast<bf16*>(p)[i] = (bf16)v; }
};

// cos, sin of 2 pi i / n from the exact rational: the index is folded to (-n / 2, n / 2], so the argument of sincospif is 2 i / n in
// [-1, 1] with one rounding (the division)
__device__ __forceinline__ void fu_sincos(int i, int n, float& c, float& s) {
  const int r = (2 * i <= n) ? i : i - n;
  sincospif((float)(2 * r) / (float)n, &s, &c);
}
__device__ __forceinline__ void fu_table(float* tab, int W) {   // tab[x] = cos tx, tab[W + x] = sin tx
  for (int x = threadIdx.x; x < W; x += FU_THREADS) fu_sincos(x, W, tab[x], tab[W + x]);
  __syncthreads();
}

// the V values of one pixel's column group; a group that straddles [lo, hi) reads the columns inside and takes 0 for the others
template <bool F32, bool FULL>
__device__ __forceinline__ void fu_load(const void* cat, size_t base, int col0, int lo, int hi, float (&v)[FuElem<F32>::V]) {
  if constexpr (FULL) {
    FuElem<F32>::load(cat, base, v);
  } else {
#pragma unroll
    for (int j = 0; j < FuElem<F32>::V; ++j) v[j] = (col0 + j >= lo && col0 + j < hi) ? FuElem<F32>::load1(cat, base + j) : 0.0f;
  }
}
template <bool F32, bool FULL>
__device__ __forceinline__ void fu_store(void* cat, size_t base, int col0, int lo, int hi, const float (&v)[FuElem<F32>::V]) {
  if constexpr (FULL) {
    FuElem<F32>::store(cat, base, v);
  } else {
#pragma unroll
    for (int j = 0; j < FuElem<F32>::V; ++j)
      if (col0 + j >= lo && col0 + j < hi) FuElem<F32>::store1(cat, base + j, v[j]);
  }
}

// the seven sums of this thread's image rows y0, y0 + ty, ... < y1 of batch item b
template <bool F32, bool FULL>
__device__ __forceinline__ void fu_sums(const void* cat, long ld, int b, int H, int W, int y0, int y1, int ty, int col0, int lo, int hi,
                                        const float* tab, float (&S)[FU_Q][FuElem<F32>::V]) {
  constexpr int V = FuElem<F32>::V;
  for (int y = y0; y < y1; y += ty) {
    float cy, sy;
    fu_sincos(y, H, cy, sy);
    float R0[V], Rc[V], Rs[V];
#pragma unroll
    for (int j = 0; j < V; ++j) R0[j] = Rc[j] = Rs[j] = 0.0f;
    const size_t row0 = ((size_t)b * H + y) * W;
#pragma unroll 4
    for (int x = 0; x < W; ++x) {
      float v[V];
      fu_load<F32, FULL>(cat, (row0 + x) * (size_t)ld + col0, col0, lo, hi, v);
      const float cx = tab[x], sx = tab[W + x];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        R0[j] += v[j];
        Rc[j] = fmaf(v[j], cx, Rc[j]);
        Rs[j] = fmaf(v[j], sx, Rs[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      S[0][j] += R0[j];
      S[1][j] = fmaf(R0[j], cy, S[1][j]);
      S[2][j] = fmaf(R0[j], sy, S[2][j]);
      S[3][j] += Rc[j];
      S[4][j] += Rs[j];
      S[5][j] += fmaf(Rc[j], cy, -(Rs[j] * sy));   // cos (ty + tx) = cy cx - sy sx
      S[6][j] += fmaf(Rc[j], sy, Rs[j] * cy);      // sin (ty + tx) = sy cx + cy sx
    }
  }
}

// grid (S.nc, splits, B); dynamic LDS: 2 W floats (tx table) + ty * gw * V floats (the block's reduction)
template <bool F32>
__global__ __launch_bounds__(FU_THREADS) void freeu_stats_kernel(const void* __restrict__ cat, long ld, int H, int W, int Cx, int Cs, FuCols S_,
                                                                 int rps, int cpad, float* __restrict__ partial) {
  constexpr int V = FuElem<F32>::V;
  extern __shared__ float fu_lds[];
  float* tab = fu_lds;
  float* red = fu_lds + 2 * W;
  fu_table(tab, W);
  const int gl = threadIdx.x % S_.gw, slot = threadIdx.x / S_.gw;
  const int g = blockIdx.x * S_.gw + gl;   // group inside the skip span
  const int split = blockIdx.y, b = blockIdx.z, nsplit = gridDim.y;
  const bool live = slot < S_.ty && g < S_.ng;
  float S[FU_Q][V];
#pragma unroll
  for (int q = 0; q < FU_Q; ++q)
#pragma unroll
    for (int j = 0; j < V; ++j) S[q][j] = 0.0f;
  if (live) {
    const int col0 = (S_.g0 + g) * V, lo = Cx, hi = Cx + Cs;
    const int y0 = split * rps + slot, y1 = min(H, (split + 1) * rps);
    if (col0 >= lo && col0 + V <= hi) fu_sums<F32, true>(cat, ld, b, H, W, y0, y1, S_.ty, col0, lo, hi, tab, S);
    else fu_sums<F32, false>(cat, ld, b, H, W, y0, y1, S_.ty, col0, lo, hi, tab, S);
  }
  float* dst = partial + ((size_t)b * nsplit + split) * FU_Q * cpad + (size_t)g * V;
#pragma unroll
  for (int q = 0; q < FU_Q; ++q) {
    if (slot < S_.ty) {
#pragma unroll
      for (int j = 0; j < V; ++j) red[(slot * S_.gw + gl) * V + j] = S[q][j];
    }
    __syncthreads();
    if (slot == 0 && g < S_.ng) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float a = red[gl * V + j];
        for (int t = 1; t < S_.ty; ++t) a += red[(t * S_.gw + gl) * V + j];   // slot order: the same sum on every run
        dst[(size_t)q * cpad + j] = a;
      }
    }
    __syncthreads();
  }
}

template <bool F32, bool FULL>
__device__ __forceinline__ void fu_scale_rows(void* cat, long ld, int b, int H, int W, int y0, int y1, int ty, int col0, int hi, float bscale) {
  constexpr int V = FuElem<F32>::V;
  for (int y = y0; y < y1; y += ty) {
    const size_t row0 = ((size_t)b * H + y) * W;
#pragma unroll 4
    for (int x = 0; x < W; ++x) {
      const size_t base = (row0 + x) * (size_t)ld + col0;
      float v[V];
      fu_load<F32, FULL>(cat, base, col0, 0, hi, v);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] *= bscale;
      fu_store<F32, FULL>(cat, base, col0, 0, hi, v);
    }
  }
}
template <bool F32, bool FULL>
__device__ __forceinline__ void fu_filter_rows(void* cat, long ld, int b, int H, int W, int y0, int y1, int ty, int col0, int lo, int hi,
                                               const float* tab, const float (&m)[FU_Q][FuElem<F32>::V]) {
  constexpr int V = FuElem<F32>::V;
  for (int y = y0; y < y1; y += ty) {
    float cy, sy;
    fu_sincos(y, H, cy, sy);
    float E[V], F[V], G[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      E[j] = fmaf(m[2][j], sy, fmaf(m[1][j], cy, m[0][j]));
      F[j] = fmaf(m[6][j], sy, fmaf(m[5][j], cy, m[3][j]));
      G[j] = fmaf(m[6][j], cy, fmaf(-m[5][j], sy, m[4][j]));
    }
    const size_t row0 = ((size_t)b * H + y) * W;
#pragma unroll 4
    for (int x = 0; x < W; ++x) {
      const size_t base = (row0 + x) * (size_t)ld + col0;
      float v[V];
      fu_load<F32, FULL>(cat, base, col0, lo, hi, v);
      const float cx = tab[x], sx = tab[W + x];
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] += fmaf(sx, G[j], fmaf(cx, F[j], E[j]));
      fu_store<F32, FULL>(cat, base, col0, lo, hi, v);
    }
  }
}

// grid (A.nc + S.nc, row chunks, B): the first A.nc grid columns scale the backbone half, the others filter the skip columns.
// dynamic LDS: 2 W floats
template <bool F32>
__global__ __launch_bounds__(FU_THREADS) void freeu_apply_kernel(void* __restrict__ cat, long ld, int H, int W, int Cx, int Cs, float bscale, float k,
                                                                 FuCols A_, FuCols S_, int rpa, int nsplit, int cpad,
                                                                 const float* __restrict__ partial) {
  constexpr int V = FuElem<F32>::V;
  extern __shared__ float fu_lds[];
  const bool filter = (int)blockIdx.x >= A_.nc;
  const FuCols f = filter ? S_ : A_;
  if (filter) fu_table(fu_lds, W);   // (block-uniform)
  const int gl = threadIdx.x % f.gw, slot = threadIdx.x / f.gw;
  const int g = ((int)blockIdx.x - (filter ? A_.nc : 0)) * f.gw + gl;
  const int b = blockIdx.z;
  if (slot >= f.ty || g >= f.ng) return;
  const int col0 = (f.g0 + g) * V;
  const int y0 = blockIdx.y * rpa + slot, y1 = min(H, ((int)blockIdx.y + 1) * rpa);
  if (!filter) {
    const int hi = Cx / 2;
    if (col0 + V <= hi) fu_scale_rows<F32, true>(cat, ld, b, H, W, y0, y1, f.ty, col0, hi, bscale);
    else fu_scale_rows<F32, false>(cat, ld, b, H, W, y0, y1, f.ty, col0, hi, bscale);
    return;
  }
  float m[FU_Q][V];   // (s - 1) x the seven means: the splits added in order
#pragma unroll
  for (int q = 0; q < FU_Q; ++q)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float* src = partial + ((size_t)b * nsplit * FU_Q + q) * cpad + (size_t)g * V + j;
      float a = src[0];
      for (int s = 1; s < nsplit; ++s) a += src[(size_t)s * FU_Q * cpad];
      m[q][j] = a * k;
    }
  const int lo = Cx, hi = Cx + Cs;
  if (col0 >= lo && col0 + V <= hi) fu_filter_rows<F32, true>(cat, ld, b, H, W, y0, y1, f.ty, col0, lo, hi, fu_lds, m);
  else fu_filter_rows<F32, false>(cat, ld, b, H, W, y0, y1, f.ty, col0, lo, hi, fu_lds, m);
}

int fu_fail(const char* msg) {
  set_last_error(msg);
  return SD_ERR_INVALID;
}
bool fu_finite(float v) { return v - v == 0.0f; }

template <bool F32>
int freeu_launch(void* cat, long ld, int B, int H, int W, int Cx, int Cs, float b, float s, float* ws, hipStream_t st) {
  constexpr int V = FuElem<F32>::V;
  const FuCols A = freeu_cols(0, Cx / 2, V), S = freeu_cols(Cx, Cx + Cs, V);
  const int cpad = S.ng * V;
  const int rps = freeu_rows_per_split(B, H, S), nsplit = (H + rps - 1) / rps;
  const size_t lds_stats = (size_t)4 * (2 * W + S.ty * S.gw * V);
  hipLaunchKernelGGL(freeu_stats_kernel<F32>, dim3(S.nc, nsplit, B), dim3(FU_THREADS), lds_stats, st, cat, ld, H, W, Cx, Cs, S, rps, cpad, ws);
  // the apply pass splits the rows the same way, sized by whichever column set has the fewer row slots per block
  const FuCols& narrow = (A.nc && A.ty < S.ty) ? A : S;
  FuCols both = narrow;
  both.nc = A.nc + S.nc;
  const int rpa = freeu_rows_per_split(B, H, both);
  const float k = (float)(((double)s - 1.0) / ((double)H * (double)W));
  hipLaunchKernelGGL(freeu_apply_kernel<F32>, dim3(A.nc + S.nc, (H + rpa - 1) / rpa, B), dim3(FU_THREADS), (size_t)8 * W, st, cat, ld, H, W, Cx, Cs,
                     b, k, A, S, rpa, nsplit, cpad, ws);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace

int launch_freeu(void* cat, int x_f32, long ld, int B, int H, int W, int Cx, int Cs, float b, float s, float* ws, hipStream_t stream) {
  if (W > FU_MAX_W || B > 65535) return SD_ERR_UNSUPPORTED;
  return x_f32 ? freeu_launch<true>(cat, ld, B, H, W, Cx, Cs, b, s, ws, stream) : freeu_launch<false>(cat, ld, B, H, W, Cx, Cs, b, s, ws, stream);
}

}  // namespace sd

extern "C" {

int64_t mi355x_sd_freeu_workspace_floats(int B, int H, int W, int Cs) { return sd::freeu_workspace_floats(B, H, W, Cs); }

int mi355x_sd_freeu(void* cat, int64_t ld, int B, int H, int W, int Cx, int Cs, float b, float s, int elem_f32, float* workspace, void* stream) {
  using namespace sd;
  if (!cat || !workspace) return fu_fail("mi355x_sd_freeu: null pointer");
  if (B < 1) return fu_fail("mi355x_sd_freeu: needs B >= 1");
  if (H < 2 || W < 2) return fu_fail("mi355x_sd_freeu: needs H >= 2 and W >= 2 (the filter scales the bins ky, kx in {-1, 0})");
  if (Cx < 0 || Cs < 1) return fu_fail("mi355x_sd_freeu: needs Cx >= 0 and Cs >= 1");
  if (ld < (int64_t)Cx + Cs) return fu_fail("mi355x_sd_freeu: ld must be at least Cx + Cs");
  const int es = elem_f32 ? 4 : 2;
  if ((reinterpret_cast<uintptr_t>(cat) & 15) || ((ld * es) & 15))
    return fu_fail("mi355x_sd_freeu: cat and the row stride (ld elements) must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return fu_fail("mi355x_sd_freeu: the workspace must be 16-byte aligned");
  if (!fu_finite(b) || !fu_finite(s)) return fu_fail("mi355x_sd_freeu: b and s must be finite");
  const int rc = launch_freeu(cat, elem_f32, (long)ld, B, H, W, Cx, Cs, b, s, workspace, reinterpret_cast<hipStream_t>(stream));
  if (rc == SD_ERR_UNSUPPORTED) set_last_error("mi355x_sd_freeu: unsupported shape (W <= 4096, B <= 65535)");
  else if (rc != SD_OK) set_last_error("mi355x_sd_freeu: HIP launch failed");
  return rc;
}

}  // extern "C"
