// InstructPix2Pix around the U-Net (gfx950, fp32 latents; ABI 24): the three-way guidance combine that writes one guided plane in front of
// the fused step tails (which take it as "already guided": eps_text == NULL), and the assembly of the 8-channel model input.
//
// Reference semantics:
//   the combine, the x0-space conversions   ppdiffusers/ppdiffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_instruct_pix2pix.py:384-409
//   rescale_noise_cfg in x0 space           pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_instruct_pix2pix.py:105-117, 903-930
//   the model input                         pipeline_stable_diffusion_instruct_pix2pix.py:373-377
#include "common.h"
#include "kernels.h"
#include "rescale_stats.h"

namespace sd {
namespace {

// The combine, per element and IN THIS ORDER (tests/ip2p_bounds.py derives its bound from it): both differences are formed first,
// each fma rounds once. The weights of t, i, u are gs, gi - gs, 1 - gi: they sum to 1.
__device__ __forceinline__ float mix3(float t, float i, float u, float gs, float gi) { return fmaf(gs, t - i, fmaf(gi, i - u, u)); }

// guidance_rescale == 0: elementwise over the n = batch * per_sample elements of a plane. nv 16-byte vectors first (0 when a pointer or
// the plane size is not 16-byte aligned), then the elements 4 * nv .. n - 1 one by one: nothing past n is read or written. The three
// planes sit n elements apart, so they are all aligned only when n % 4 == 0: the launcher passes nv = n / 4 (the second loop then
// has no element left) or nv = 0 (the first has none). A launch runs one loop or the other, never a vector pass with a remainder.
__global__ void guidance3_flat_kernel(const float* __restrict__ et, const float* __restrict__ ei, const float* __restrict__ eu,
                                      float* __restrict__ out, float gs, float gi, long nv, long n) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  const f32x4 *t4 = reinterpret_cast<const f32x4*>(et), *i4 = reinterpret_cast<const f32x4*>(ei), *u4 = reinterpret_cast<const f32x4*>(eu);
  for (long i = gid; i < nv; i += stride) {
    const f32x4 tv = t4[i], iv = i4[i], uv = u4[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = mix3(tv[j], iv[j], uv[j], gs, gi);
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
  for (long i = 4 * nv + gid; i < n; i += stride) out[i] = mix3(et[i], ei[i], eu[i], gs, gi);
}

// guidance_rescale > 0: one block of CRA_THREADS threads per sample of n elements, no scratch. With (t, i, u) the sample's three model
// outputs -- X0: their predicted originals p = fma(-sigma, e, x), sigma = coef[0] read from device memory -- and c = mix3(t, i, u):
//   k = gr * std(t) / std(c) + (1 - gr)       the statistics as cfg_rescale_factor (step_tail.hip) takes them: each variance by two
//                                             passes, every sum a fixed tree (a lane adds its elements tid, tid + 1024, ... in order,
//                                             then block_sum2), no atomics, the same bits in every lane; nothing is added to a zero variance
//   out = c * k                               X0: out = (c * k - x) / (-sigma)
// RESIDENT (n <= CRA_THREADS * CRA_RES): a lane keeps its t and c in registers and the planes are read once; larger samples are read
// three times, the second and third time from L2. plane = batch * n, the distance between the three outputs of one sample.
template <bool X0, bool RESIDENT>
__global__ __launch_bounds__(CRA_THREADS) void guidance3_rescale_kernel(const float* __restrict__ eps, const float* __restrict__ x,
                                                                        const float* __restrict__ coef, float* __restrict__ out, float gs,
                                                                        float gi, float gr, long n, long plane) {
  __shared__ float part[2][CRA_THREADS / 64];
  const long base = (long)blockIdx.x * n;
  const float *et = eps + base, *ei = et + plane, *eu = ei + plane;
  out += base;
  float nsig = 0.f;
  if (X0) {
    x += base;
    nsig = -coef[0];
  }
  const int tid = threadIdx.x;
  auto load = [&](long i, float& t, float& c) {
    float a = et[i], b = ei[i], u = eu[i];
    if (X0) {
      const float xv = x[i];
      a = fmaf(nsig, a, xv), b = fmaf(nsig, b, xv), u = fmaf(nsig, u, xv);
    }
    t = a;
    c = mix3(a, b, u, gs, gi);
  };
  constexpr int R = RESIDENT ? CRA_RES : 1;
  float tv[R], cv[R];
  float s_t = 0.f, s_c = 0.f;
  if (RESIDENT) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = tid + j * CRA_THREADS;
      tv[j] = cv[j] = 0.f;
      if (i < n) {
        load(i, tv[j], cv[j]);
        s_t += tv[j];
        s_c += cv[j];
      }
    }
  } else {
    for (long i = tid; i < n; i += CRA_THREADS) {
      float t, c;
      load(i, t, c);
      s_t += t;
      s_c += c;
    }
  }
  block_sum2(s_t, s_c, part);
  const float inv_n = 1.0f / (float)n;
  const float m_t = s_t * inv_n, m_c = s_c * inv_n;
  float q_t = 0.f, q_c = 0.f;
  if (RESIDENT) {
#pragma unroll
    for (int j = 0; j < R; ++j)
      if (tid + j * CRA_THREADS < n) {
        const float dt = tv[j] - m_t, dc = cv[j] - m_c;
        q_t += dt * dt;
        q_c += dc * dc;
      }
  } else {
    for (long i = tid; i < n; i += CRA_THREADS) {
      float t, c;
      load(i, t, c);
      const float dt = t - m_t, dc = c - m_c;
      q_t += dt * dt;
      q_c += dc * dc;
    }
  }
  block_sum2(q_t, q_c, part);
  const float inv_nm1 = 1.0f / (float)(n - 1);
  const float r = sqrtf(q_t * inv_nm1) / sqrtf(q_c * inv_nm1);
  const float k = gr * r + (1.0f - gr);
  auto store = [&](long i, float c) {
    float v = c * k;
    if (X0) v = (v - x[i]) / nsig;
    out[i] = v;
  };
  if (RESIDENT) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = tid + j * CRA_THREADS;
      if (i < n) store(i, cv[j]);
    }
  } else {
    for (long i = tid; i < n; i += CRA_THREADS) {
      float t, c;
      load(i, t, c);
      store(i, c);
    }
  }
}

// One output sample (blockIdx.y = g * batch + b) is two contiguous runs: la = c_lat * hw elements scale * x[b], then lb = c_img * hw
// elements of image_latents[g * batch + b]. VEC: both runs and all three pointers are multiples of 16 bytes, an element is a f32x4.
template <bool VEC>
__global__ void ip2p_input_kernel(const float* __restrict__ x, const float* __restrict__ img, float* __restrict__ out, float scale,
                                  int batch, long la, long lb) {
  const long s = blockIdx.y;
  const float *xs = x + (s % batch) * la, *is = img + s * lb;
  float* o = out + s * (la + lb);
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  if (VEC) {
    const long na = la / 4, nt = (la + lb) / 4;
    for (long i = gid; i < nt; i += stride) {
      f32x4 v;
      if (i < na) {
        v = reinterpret_cast<const f32x4*>(xs)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= scale;
      } else {
        v = reinterpret_cast<const f32x4*>(is)[i - na];
      }
      reinterpret_cast<f32x4*>(o)[i] = v;
    }
  } else {
    for (long i = gid; i < la + lb; i += stride) o[i] = i < la ? xs[i] * scale : is[i - la];
  }
}

}  // namespace

int launch_guidance3(const float* eps, const float* x, const float* coef, float* out, float gs, float gi, float gr, int batch,
                     long per_sample, hipStream_t stream) {
  if (batch <= 0 || per_sample < 1) return SD_ERR_INVALID;
  const long n = (long)batch * per_sample;
  if (gr > 0.0f) {
    if (per_sample < 2 || (x && !coef)) return SD_ERR_INVALID;
    const bool res = per_sample <= (long)CRA_THREADS * CRA_RES;
    const auto kernel = x ? (res ? guidance3_rescale_kernel<true, true> : guidance3_rescale_kernel<true, false>)
                          : (res ? guidance3_rescale_kernel<false, true> : guidance3_rescale_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(CRA_THREADS), 0, stream, eps, x, coef, out, gs, gi, gr, per_sample, n);
  } else {
    // (the three planes are n elements apart: all of them 16-byte aligned only when n is a multiple of 4)
    const long nv = ((((uintptr_t)eps | (uintptr_t)out) & 15) || (n & 3)) ? 0 : n / 4;
    const long work = nv > n - 4 * nv ? nv : n - 4 * nv;
    long nb = (work + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(guidance3_flat_kernel, dim3((unsigned)nb), dim3(256), 0, stream, eps, eps + n, eps + 2 * n, out, gs, gi, nv, n);
  }
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

int launch_ip2p_input(const float* x, const float* img, float* out, float scale, int groups, int batch, int c_lat, int c_img, long hw,
                      hipStream_t stream) {
  if (groups < 1 || batch < 1 || c_lat < 1 || c_img < 1 || hw < 1) return SD_ERR_INVALID;
  const long samples = (long)groups * batch, la = (long)c_lat * hw, lb = (long)c_img * hw;
  if (samples > 65535) return SD_ERR_UNSUPPORTED;
  const bool vec = !((la | lb) & 3) && !(((uintptr_t)x | (uintptr_t)img | (uintptr_t)out) & 15);
  const long work = vec ? (la + lb) / 4 : la + lb;
  long nb = (work + 1023) / 1024;   // up to four elements per thread before the grid stride repeats
  if (nb > 256) nb = 256;
  const auto kernel = vec ? ip2p_input_kernel<true> : ip2p_input_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nb, (unsigned)samples), dim3(256), 0, stream, x, img, out, scale, batch, la, lb);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
