// Semantic guidance (SEGA) between the U-Net and the fused step tails (gfx950, fp32 latents; ABI 25): ONE launch writes the guided
// plane that every step-tail entry takes as "already guided" (eps_text == NULL) and updates the momentum plane in place.
//
// Reference semantics:  ppdiffusers/ppdiffusers/pipelines/semantic_stable_diffusion/pipeline_semantic_stable_diffusion.py:541-699
//   per concept  g = (e_c - u) * (+-scale);  thr = quantile(|g| over the H*W plane of each (sample, channel), threshold);
//                g_c = where(|g| >= thr, g, 0)                                                                   (:615-649)
//   then the warm-up regimes, the momentum and the sums of :654-699 (include/mi355x_sd.h states them per element).
//
// The quantile is an ORDER STATISTIC, and it is taken exactly: the keys are the bit patterns of |g|, which order as unsigned
// integers; a radix select (4 digits of 8 bits, most significant first, a 256-bin histogram in LDS, integer LDS atomics -- counts are
// exact in any order) finds the key of rank lo, the count of its equals tells whether rank lo + 1 is the same key, and if not one
// integer-min pass finds the smallest key above it. No floating-point value is ever reduced across elements.
//
// Launch shape: one block of 1024 threads per (sample, channel); the block selects for its n concepts one
// after the other and then makes the one elementwise pass over its plane. The keys are NOT kept in LDS: every digit pass recomputes
// |g| from the two planes it is made of, which a plane of <= 65536 elements keeps in L2 (2 x 256 KB at most), so LDS holds the
// histogram only (1 KB), there is ONE form of the kernel for every plane size, and the recomputed keys are the mask's own bits.
#include "common.h"
#include "kernels.h"

namespace sd {
namespace {

constexpr int SEGA_THREADS = 1024;
constexpr int SEGA_MAX_CONCEPTS = 8;
constexpr long SEGA_MAX_HW = 65536;
// a row of the per-step table (32-bit words; paddlemix_amd/sega_forms.py builds it, include/mi355x_sd.h states it)
enum { R_REGIME = 0, R_ACTIVE = 1, R_WARM = 2, R_GS = 4, R_MS = 5, R_BETA = 6, R_OMB = 7, R_HEAD = 8 };
enum { C_SCALE = 0, C_LO = 1, C_FRAC = 2, C_WFULL = 3, C_WPART = 4, C_WORDS = 5 };
enum { REGIME_NONE = 0, REGIME_PARTIAL = 1, REGIME_ALL = 2 };

// g of one element: a subtraction, then a multiplication -- two roundings, nothing to contract
__device__ __forceinline__ float edit_dir(float e, float u, float s) { return (e - u) * s; }
__device__ __forceinline__ unsigned key_of(float g) { return __float_as_uint(g) & 0x7fffffffu; }

// torch.lerp as its vectorised CPU kernel takes it: the weight decides which end the difference is added to, by one fma
//   w < 0.5: fma(w, b - a, a)      otherwise: fma(w - 1, b - a, b)        (w - 1 is exact for w in [0.5, 1))
__device__ __forceinline__ float lerp_torch(float a, float b, float w) {
  const float diff = b - a;
  return fabsf(w) < 0.5f ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);
}

// f(key) for every element of the plane; VEC: the plane's pointers are 16-byte aligned and hw % 4 == 0
template <bool VEC, class F>
__device__ __forceinline__ void for_keys(const float* __restrict__ e, const float* __restrict__ u, float s, int hw, F f) {
  if (VEC) {
    const f32x4 *e4 = reinterpret_cast<const f32x4*>(e), *u4 = reinterpret_cast<const f32x4*>(u);
    for (int i = threadIdx.x; i < hw / 4; i += SEGA_THREADS) {
      const f32x4 ev = e4[i], uv = u4[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) f(key_of(edit_dir(ev[j], uv[j], s)));
    }
  } else {
    for (int i = threadIdx.x; i < hw; i += SEGA_THREADS) f(key_of(edit_dir(e[i], u[i], s)));
  }
}

struct SelectShared {
  unsigned hist[256];
  unsigned bin, rank, count, minkey, nan;
  float thr[SEGA_MAX_CONCEPTS];
};

// After a histogram pass: wave 0 finds the bin in which the running count passes `rank` (0 <= rank < the histogram's total), the rank
// inside that bin and the bin's count. A lane owns four consecutive bins; an inclusive scan over the 64 lanes by shuffles.
__device__ __forceinline__ void pick_bin(SelectShared& sh, unsigned rank) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned c0 = sh.hist[4 * lane], c1 = sh.hist[4 * lane + 1], c2 = sh.hist[4 * lane + 2], c3 = sh.hist[4 * lane + 3];
    const unsigned own = c0 + c1 + c2 + c3;
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    const unsigned excl = incl - own;
    if (rank >= excl && rank < incl) {   // exactly one lane
      unsigned r = rank - excl, b = 4 * lane, c = c0;
      if (r >= c0) {
        r -= c0, ++b, c = c1;
        if (r >= c1) {
          r -= c1, ++b, c = c2;
          if (r >= c2) r -= c2, ++b, c = c3;
        }
      }
      sh.bin = b, sh.rank = r, sh.count = c;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(SEGA_THREADS) void sega_guidance_kernel(const float* __restrict__ eps, float* __restrict__ momentum,
                                                                     const float* __restrict__ extra, const float* __restrict__ row,
                                                                     float* __restrict__ out, float* __restrict__ stats, int n, int batch,
                                                                     int channels, int hw) {
  __shared__ SelectShared sh;
  const int tid = threadIdx.x;
  const long plane = blockIdx.x;                               // sample * channels + channel
  const long group = (long)batch * channels * hw;              // the distance between u, t, e_0, ...
  const float* u = eps + plane * hw;
  const float* t = u + group;
  const unsigned* rowi = reinterpret_cast<const unsigned*>(row);
  const unsigned active = rowi[R_ACTIVE];

  for (int c = 0; c < n; ++c) {
    const float* rc = row + R_HEAD + c * C_WORDS;
    float* st = stats ? stats + 3 * ((long)c * batch * channels + plane) : nullptr;
    if (!((active >> c) & 1u)) {                               // cooled down: g_c = 0, no selection
      if (tid == 0) {
        sh.thr[c] = 0.0f;
        if (st) st[0] = st[1] = st[2] = 0.0f;
      }
      continue;
    }
    const float s = rc[C_SCALE], frac = rc[C_FRAC];
    int lo = (int)reinterpret_cast<const unsigned*>(rc)[C_LO];
    lo = lo < 0 ? 0 : (lo > hw - 1 ? hw - 1 : lo);             // a rank, never an index: clamped so that one bin always matches
    const bool two = frac != 0.0f && lo + 1 <= hw - 1;         // hi = ceil(rank) = lo + 1
    const float* e = eps + (2 + c) * group + plane * hw;

    unsigned prefix = 0, mask = 0, rank = (unsigned)lo;
    if (tid == 0) sh.nan = 0u;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) sh.hist[tid] = 0u;
      __syncthreads();
      for_keys<VEC>(e, u, s, hw, [&](unsigned k) {
        if ((k & mask) == prefix) atomicAdd(&sh.hist[(k >> shift) & 255u], 1u);
        if (shift == 24 && k > 0x7f800000u) sh.nan = 1u;       // (every writer writes the same value)
      });
      __syncthreads();
      pick_bin(sh, rank);
      __syncthreads();
      prefix |= sh.bin << shift;
      mask |= 255u << shift;
      rank = sh.rank;
    }
    // prefix is the key of rank lo; sh.count keys equal it, rank of them sit below position lo
    unsigned key_hi = prefix;
    if (two && rank + 1 >= sh.count) {                         // rank lo + 1 is past the equals: the smallest key above
      if (tid == 0) sh.minkey = 0xffffffffu;
      __syncthreads();
      for_keys<VEC>(e, u, s, hw, [&](unsigned k) {
        if (k > prefix) atomicMin(&sh.minkey, k);
      });
      __syncthreads();
      key_hi = sh.minkey;
    }
    if (tid == 0) {
      const float vlo = __uint_as_float(prefix), vhi = __uint_as_float(key_hi);
      const float thr = sh.nan ? __uint_as_float(0x7fc00000u) : lerp_torch(vlo, vhi, frac);   // a NaN in the plane: a NaN quantile
      sh.thr[c] = thr;
      if (st) st[0] = vlo, st[1] = vhi, st[2] = thr;
    }
    __syncthreads();   // (also keeps the next concept's first writes behind this one's last reads)
  }
  __syncthreads();

  // ---- the one elementwise pass: out and momentum of this plane, the concepts summed in index order
  const int regime = (int)rowi[R_REGIME];
  const unsigned warm = rowi[R_WARM];
  const float gs = row[R_GS], ms = row[R_MS], beta = row[R_BETA], omb = row[R_OMB];
  float sc[SEGA_MAX_CONCEPTS], wf[SEGA_MAX_CONCEPTS], wp[SEGA_MAX_CONCEPTS], th[SEGA_MAX_CONCEPTS];
#pragma unroll
  for (int c = 0; c < SEGA_MAX_CONCEPTS; ++c)
    if (c < n) {
      const float* rc = row + R_HEAD + c * C_WORDS;
      sc[c] = rc[C_SCALE], wf[c] = rc[C_WFULL], wp[c] = rc[C_WPART], th[c] = sh.thr[c];
    }
  float* mom = momentum + plane * hw;
  const float* ex = extra ? extra + plane * hw : nullptr;
  float* o = out + plane * hw;
  for (int i = tid; i < hw; i += SEGA_THREADS) {
    const float uv = u[i];
    float guid = gs * (t[i] - uv);
    float edit = 0.0f, part = 0.0f;
#pragma unroll
    for (int c = 0; c < SEGA_MAX_CONCEPTS; ++c)
      if (c < n) {
        float g = 0.0f;
        if ((active >> c) & 1u) {
          const float d = edit_dir(eps[(2 + c) * group + plane * hw + i], uv, sc[c]);
          g = fabsf(d) >= th[c] ? d : 0.0f;                    // (a NaN threshold compares false)
        }
        edit = fmaf(wf[c], g, edit);
        if ((warm >> c) & 1u) part = fmaf(wp[c], g, part);
      }
    if (regime == REGIME_PARTIAL) guid = guid + part;
    const float m = mom[i];
    edit = fmaf(ms, m, edit);
    mom[i] = fmaf(beta, m, omb * edit);
    if (regime == REGIME_ALL) guid = guid + edit;
    if (ex) guid = guid + ex[i];
    o[i] = uv + guid;
  }
}

}  // namespace

int launch_sega_guidance(const float* eps, float* momentum, const float* extra, const float* row, float* out, float* stats, int n,
                         int batch, int channels, long hw, hipStream_t stream) {
  if (n < 1 || batch < 1 || channels < 1 || hw < 1) return SD_ERR_INVALID;
  if (n > SEGA_MAX_CONCEPTS || hw > SEGA_MAX_HW || (long)batch * channels > 0x7fffffffL) return SD_ERR_UNSUPPORTED;
  // every plane starts hw floats after the one before: all of them 16-byte aligned only when the base is and hw % 4 == 0
  const bool vec = !(hw & 3) && !(((uintptr_t)eps) & 15);
  const auto kernel = vec ? sega_guidance_kernel<true> : sega_guidance_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(batch * channels)), dim3(SEGA_THREADS), 0, stream, eps, momentum, extra, row, out, stats, n,
                     batch, channels, (int)hw);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
