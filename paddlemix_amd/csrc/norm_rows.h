// The row-normalisation skeleton (gfx950): "one wave owns a row in registers". LayerNorm, the LayerNorm row statistics, adaLN and
// adaLN + e4m3 (norm.hip) are one kernel, row_norm_kernel, over four forms; RMSNorm (norm.hip) and the fused adaLN + scale + residual
// op (fused_ops.hip) keep bodies of their own on the same pieces (RowWave, the loads, row_moments / row_rms, store8) and go through
// the same launcher (RowKernel): why, at each of them and in DESIGN.md, "Adding a row-normalisation form".
//
// A ROW FORM is a small struct, passed by value, that holds the operand pointers of its kernel and states what is its own:
//   Chunk               what a lane keeps of 8 consecutive channels: 8 floats, or the raw 16-byte vector
//   keep<NCH>(w)        what a wave keeps over all its rows (LayerNorm: gamma / beta of its chunks); most forms keep Nothing
//   load(row, v, w)     the row's NCH chunks as the values the statistics see (load_row); zeros past the row's end
//   finish(row, v, mean, rstd, w, kept)    the finished row: affine or modulation and the store, or the statistics themselves
// The skeleton owns the rest: the wave-walks-rows loop with its clamped load row and its store guard, the statistics over ROWS rows
// with their butterflies interleaved, and on the host launch_row_norm: the choice of NCH, the launch and the route line. A form is a
// template argument: each instantiation inlines to a kernel of its own, with no call and no switch on the form at run time.
#pragma once
#include "common.h"
#include "kernels.h"

namespace sd {

// 8 consecutive channels of a row as fp32: from the build's 16-bit elements (one 16-byte load) or, in the fp32
// residual-stream mode (XF32), from fp32 rows (two 16-byte loads). `x` is the row base in ELEMENTS of its own type.
// `ok == false` yields zeros. Only the raw load sits under the predicate (the conversion does not), so that the compiler
// issues the loads of an unrolled caller back to back instead of one branch + s_waitcnt per chunk.
template <bool XF32>
__device__ __forceinline__ void load8f(const void* x, size_t elem_off, float (&f)[8], bool ok = true) {
  if constexpr (XF32) {
    const float* p = reinterpret_cast<const float*>(x) + elem_off;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      a = *reinterpret_cast<const f32x4*>(p);
      b = *reinterpret_cast<const f32x4*>(p + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
  } else {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (ok) raw = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16*>(x) + elem_off);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(&raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
  }
}

struct RowWave {   // a lane's place in its wave's rows: chunk i of the lane is channels 8 * (lane + 64 * i) ..., valid while below cv
  int lane, cv;
  float invC;
  __device__ explicit RowWave(int C) : lane(threadIdx.x & 63), cv(C >> 3), invC(1.0f / (float)C) {}
};
struct Nothing {};

// a lane's NCH chunks of the row that starts at element row_off of x, under one predicate each: as 8 floats, or as the raw vector
template <bool XF32, int NCH>
__device__ __forceinline__ void load_row(const void* x, size_t row_off, float (&v)[NCH][8], const RowWave& w) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cc = w.lane + 64 * i;
    load8f<XF32>(x, row_off + cc * 8, v[i], cc < w.cv);
  }
}
template <int NCH>
__device__ __forceinline__ void load_row(const bf16* x, size_t row_off, u32x4 (&v)[NCH], const RowWave& w) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cc = w.lane + 64 * i;
    v[i] = u32x4{0u, 0u, 0u, 0u};
    if (cc < w.cv) v[i] = *reinterpret_cast<const u32x4*>(x + row_off + cc * 8);
  }
}

// 8 fp32 values -> 8 elements of the build's type, as one 16-byte vector / stored with one 16-byte store
__device__ __forceinline__ u32x4 pack8(const float (&o)[8]) {
  return u32x4{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7])};
}
__device__ __forceinline__ void store8(bf16* p, const float (&o)[8]) { *reinterpret_cast<u32x4*>(p) = pack8(o); }

// element j of a chunk, whichever way the form keeps it
__device__ __forceinline__ float chunk_val(const float (&c)[8], int j) { return c[j]; }
__device__ __forceinline__ float chunk_val(const u32x4& c, int j) { return (float)__builtin_bit_cast(bf16x8, c)[j]; }

// mean and 1 / sqrt(var + eps) of ROWS rows, in every lane. One pass over data shifted by the row's first element K (the pilot):
// sum(x - K), sum((x - K)^2) -- no cancellation for the O(1..10) activations here, and none however large |mean| / std is
// (tests/test_norm_bounds.py); biased variance, fp32. The ROWS reduction chains interleave; one row's chain is wave_sum's.
template <int ROWS, int NCH, class T>
__device__ __forceinline__ void row_moments(const T (&v)[ROWS][NCH], const RowWave& w, float eps, float (&mean)[ROWS],
                                            float (&rstd)[ROWS]) {
  float s1[ROWS], s2[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const float K = __shfl(chunk_val(v[r][0], 0), 0, 64);
    float a = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if (w.lane + 64 * i < w.cv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = chunk_val(v[r][i], j) - K;
          a += d;
          q = __builtin_fmaf(d, d, q);
        }
      }
    }
    s1[r] = a;
    s2[r] = q;
    mean[r] = K;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      s1[r] += __shfl_xor(s1[r], o, 64);
      s2[r] += __shfl_xor(s2[r], o, 64);
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const float m = s1[r] * w.invC;
    const float var = fmaxf(s2[r] * w.invC - m * m, 0.f);
    mean[r] += m;
    rstd[r] = rsqrtf(var + eps);
  }
}

// RMSNorm's statistics: rstd = 1 / sqrt(mean(x^2) + eps) of ROWS rows from each lane's sum of squares (no mean subtraction)
template <int ROWS>
__device__ __forceinline__ void row_rms(float (&ss)[ROWS], const RowWave& w, float eps, float (&rstd)[ROWS]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) ss[r] += __shfl_xor(ss[r], o, 64);
#pragma unroll
  for (int r = 0; r < ROWS; ++r) rstd[r] = rsqrtf(ss[r] * w.invC + eps);
}

// Persistent waves: a wave walks rows, ROWS at a time -- all loads issued up front, the ROWS reduction chains interleave -- so the
// per-row traffic is exactly what the form reads and writes of the row. The rows of the last trip that lie past the end load
// the last row again (clamped) and are not finished.
template <class Form, int NCH, int ROWS>
__global__ __launch_bounds__(256) void row_norm_kernel(Form f, int rows, int C, float eps) {
  const RowWave w(C);
  const int wave_g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  const auto kept = f.template keep<NCH>(w);
  for (int row0 = wave_g * ROWS; row0 < rows; row0 += nwaves * ROWS) {
    typename Form::Chunk v[ROWS][NCH];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) f.load(ROWS > 1 ? min(row0 + r, rows - 1) : row0, v[r], w);
    float mean[ROWS], rstd[ROWS];
    row_moments(v, w, eps, mean, rstd);
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      if (row0 + r < rows) f.finish(row0 + r, v[r], mean[r], rstd[r], w, kept);
  }
}

// ---- host: the three grid rules, and the one launcher --------------------------------------------------------------------------
// Grid of the LayerNorm-class kernels: blocks = clamp(needed / div, min, max). Round 1 measured, back to back in isolation,
// that waves walking 2-4 row groups beat one group per wave (scripts/ln_probe.py: 8192 x 1280 15.7 -> 13.6 us at 256 blocks) and
// used div = 2; inside the SDXL step, and with the per-wave prologue now 12 vector loads instead of 48 branches, one trip per
// wave wins (LayerNorm class 3.07 -> 2.79 ms per step, profiles/r02_k_ln_grid.txt): div = 1, at most 1024 blocks.
inline int ln_grid(int rows, int rows_per_block) {
  constexpr int lo = 256, hi = 1024;   // (div = 1)
  const int needed = (rows + rows_per_block - 1) / rows_per_block;
  int blocks = needed;
  if (blocks < lo) blocks = lo;
  if (blocks > hi) blocks = hi;
  return blocks < needed ? blocks : needed;
}
// adaLN: all groups of 16 rows resident (measured better here than the capped grid of ln_grid: 2.54 vs 2.77 ms per SD3 step --
// the per-batch scale / shift vectors add a dependent load to every iteration)
inline int adaln_grid(int rows) { return (rows + 15) / 16 < 2048 ? (rows + 15) / 16 : 2048; }
// the one-row-per-wave kernels (adaLN + e4m3, the fused op): four rows per block
inline int one_row_grid(int rows) { return (rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048; }

template <int NCH_, int ROWS_>
struct Inst {   // an instantiation an entry supports: rows of up to 64 * NCH chunks, ROWS of them per trip
  static constexpr int NCH = NCH_, ROWS = ROWS_;
};
// the kernel of a form: the skeleton, unless the form's file specialises this for a body of its own (same parameters)
template <class Form, int NCH, int ROWS>
struct RowKernel {
  static constexpr auto fn = row_norm_kernel<Form, NCH, ROWS>;
};

template <class I, class Form>
bool launch_if_covers(const Form& f, int rows, int C, float eps, int blocks, const char* entry, const char* flags, hipStream_t stream) {
  if ((C >> 3) > 64 * I::NCH) return false;
  hipLaunchKernelGGL((RowKernel<Form, I::NCH, I::ROWS>::fn), dim3(blocks), dim3(256), 0, stream, f, rows, C, eps);
  norm_route(entry, C, I::NCH, I::ROWS, flags);
  return true;
}
// Launches the first of the entry's instantiations whose NCH chunks per lane cover the row, on `blocks` blocks of 4 waves, and logs
// the route "entry C NCH ROWS flags". A row that none covers is SD_ERR_UNSUPPORTED (the callers' own checks refuse it earlier).
template <class... Insts, class Form>
int launch_row_norm(const Form& f, int rows, int C, float eps, int blocks, const char* entry, const char* flags, hipStream_t stream) {
  if (!(launch_if_covers<Insts>(f, rows, C, eps, blocks, entry, flags, stream) || ...)) return SD_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
