// The fused step tails (gfx950): the guidance combine, the guidance rescale and one scheduler step in one launch over the fp32 latents.
//
// One skeleton, eight step forms. A STEP FORM is a small struct -- LinearStep (DDIM at eta = 0, Euler), MultistepStep (DPM-Solver
// multistep), UniPCStep, AncestralStep (Euler a), HeunStep (Heun: two stages), MidpointStep (DPM2 and DPM2 a: two stages, the second
// with noise), PlmsStep (PNDM's PLMS: a ring of three model outputs and a parked sample), SinglestepStep (DPM-Solver singlestep: a
// parked sample and the group's first two converted outputs) -- that holds the operand pointers of its step and states its
// arithmetic once:
//   operands            the leading members, filled by the public launcher (aggregate initialisation; the rest is set on the device)
//   FLAT                whether the form has an elementwise kernel here (LinearStep: no, see there)
//   vector_ok()         host: the operands allow the 16-byte vector loop (alignment, and whatever else the form needs)
//   load(coef)          device: the coefficients from device memory, once, and the uniform predicates derived from them
//   to_sample(base)     device: move the operands to the sample that starts at element `base`
//   elem(i, e)          device: element i, given its guided (and rescaled) model output e
//   vec(i, guided)      device: the four elements of 16-byte vector i: vector loads, the same arithmetic per lane. guided() gives their
//                       four e; a form loads x first and calls it second -- the order of the loads decides which product of a sum
//                       the compiler's packed math contracts into an fma, and this order keeps the bits of the hand-written kernels
// The skeleton owns everything else: step_flat_kernel the vector loop, the scalar remainder, the eu / et loads and cfg_mix;
// step_rescale_kernel the per-sample statistics and the RESIDENT / strided last pass; launch_step the choice between them, the
// alignment mask and the grid. A form is a template argument: each instantiation inlines to a kernel of its own, with no call and no
// switch on the form at run time.
//
// Reference semantics:
//   guidance combine, rescale_noise_cfg  ppdiffusers/ppdiffusers/pipelines/stable_diffusion/pipeline_stable_diffusion.py:69-80, 882-891
//   the steps                            schedulers/scheduling_euler_discrete.py, scheduling_ddim.py, scheduling_dpmsolver_multistep.py,
//                                        scheduling_unipc_multistep.py, scheduling_euler_ancestral_discrete.py,
//                                        scheduling_heun_discrete.py, scheduling_k_dpm_2_discrete.py,
//                                        scheduling_k_dpm_2_ancestral_discrete.py, scheduling_pndm.py (step_plms),
//                                        scheduling_dpmsolver_singlestep.py
#include "common.h"
#include "kernels.h"
#include "rescale_stats.h"

namespace sd {

// The guidance rescale (rescale_noise_cfg): per sample
//   c = eu + gs * (et - eu),  r = std(et) / std(c) over the sample's n elements,  e = c * (gr * r + 1 - gr).
// One block of 1024 threads per sample, no scratch. Each variance takes two passes (the mean, then the squared deviations from it; a
// latent with an offset would cancel in sum(v^2) - n mean^2). Every sum is a fixed tree: a lane adds its elements tid, tid + 1024, ...
// in that order, the 64 lanes of a wave fold by butterfly (wave_sum), the 16 wave partials go through LDS and fold by a second,
// four-level butterfly -- no atomics, and every lane ends with the same bits. Nothing is added to a zero variance.
// A block of 1024 threads has 128 registers per lane (16 waves on 4 SIMDs of 512), so a lane keeps CRA_RES = 32 values of et and 32 of
// c in registers: samples of up to CRA_THREADS * CRA_RES = 32768 elements are read from memory once (RESIDENT); larger ones (the
// 4 x 128 x 128 SDXL latent is 65536) read eu / et three times, the second and third time from L2 (<= 2 MB per step: latency, not
// bandwidth). The step's own operands are read and written by the same lane in the last pass only, so out may be x.
// (CRA_THREADS, CRA_RES and block_sum2, the block-wide pair of sums: rescale_stats.h, shared with ip2p.hip)

__device__ __forceinline__ float cfg_mix(float u, float t, float gs) { return fmaf(gs, t - u, u); }

// The statistics passes of a sample: k = gr * std(et) / std(c) + (1 - gr), the same bits in every lane. RESIDENT: cv[j] <- c of the
// lane's element tid + j * CRA_THREADS (0 past n), kept for the caller's last pass.
template <bool RESIDENT>
__device__ __forceinline__ float cfg_rescale_factor(const float* __restrict__ eu, const float* __restrict__ et, float gs, float gr,
                                                    long n, float (&cv)[RESIDENT ? CRA_RES : 1], float (*part)[CRA_THREADS / 64]) {
  const int tid = threadIdx.x;
  constexpr int R = RESIDENT ? CRA_RES : 1;
  float tv[R];
  float s_t = 0.f, s_c = 0.f;
  if (RESIDENT) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = tid + j * CRA_THREADS;
      tv[j] = cv[j] = 0.f;
      if (i < n) {
        tv[j] = et[i];
        cv[j] = cfg_mix(eu[i], tv[j], gs);
        s_t += tv[j];
        s_c += cv[j];
      }
    }
  } else {
    for (long i = tid; i < n; i += CRA_THREADS) {
      const float t = et[i];
      s_t += t;
      s_c += cfg_mix(eu[i], t, gs);
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
      const float t = et[i];
      const float dt = t - m_t, dc = cfg_mix(eu[i], t, gs) - m_c;
      q_t += dt * dt;
      q_c += dc * dc;
    }
  }
  block_sum2(q_t, q_c, part);
  const float inv_nm1 = 1.0f / (float)(n - 1);
  const float r = sqrtf(q_t * inv_nm1) / sqrtf(q_c * inv_nm1);
  return gr * r + (1.0f - gr);
}

// gr == 0 (or no guidance): elementwise over the n = batch * per_sample elements. nv 16-byte vectors first (0 when vector_ok() fails:
// a pointer or a plane is not 16-byte aligned), then the elements 4 * nv .. n - 1 one by one: nothing past n is read or written.
// e = eu (no guidance) or cfg_mix(eu, et, gs).
template <class Step, bool CFG>
__global__ void step_flat_kernel(Step s, const float* __restrict__ eu, const float* __restrict__ et, const float* __restrict__ coef,
                                 float gs, long nv, long n) {
  s.load(coef);
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  const f32x4 *u4 = reinterpret_cast<const f32x4*>(eu), *t4 = reinterpret_cast<const f32x4*>(et);
  for (long i = gid; i < nv; i += stride) {
    s.vec(i, [&] {
      f32x4 ev = u4[i];
      if (CFG) {
        const f32x4 tv = t4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = cfg_mix(ev[j], tv[j], gs);
      }
      return ev;
    });
  }
  for (long i = 4 * nv + gid; i < n; i += stride) {
    const float u = eu[i];
    s.elem(i, CFG ? cfg_mix(u, et[i], gs) : u);
  }
}

// gr > 0: one block per sample of n elements, the statistics (cfg_rescale_factor), then the step in the last pass with
// e = cfg_mix(eu, et, gs) * k.
template <class Step, bool RESIDENT>
__global__ __launch_bounds__(CRA_THREADS) void step_rescale_kernel(Step s, const float* __restrict__ eu, const float* __restrict__ et,
                                                                   const float* __restrict__ coef, float gs, float gr, long n) {
  __shared__ float part[2][CRA_THREADS / 64];
  const long base = (long)blockIdx.x * n;
  eu += base, et += base;
  s.load(coef);
  s.to_sample(base);
  const int tid = threadIdx.x;
  constexpr int R = RESIDENT ? CRA_RES : 1;
  float cv[R];
  const float k = cfg_rescale_factor<RESIDENT>(eu, et, gs, gr, n, cv, part);
  if (RESIDENT) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = tid + j * CRA_THREADS;
      if (i < n) s.elem(i, cv[j] * k);
    }
  } else {
    for (long i = tid; i < n; i += CRA_THREADS) s.elem(i, cfg_mix(eu[i], et[i], gs) * k);
  }
}

// The one dispatch: the rescale kernel (a form without a flat kernel: always), RESIDENT up to CRA_THREADS * CRA_RES elements per
// sample; else the flat kernel, with or without guidance.
template <class Step>
int launch_step(const Step& s, const float* eu, const float* et, const float* coef, float gs, float gr, int batch, long per_sample,
                hipStream_t stream) {
  if (batch <= 0 || per_sample < 1) return SD_ERR_INVALID;
  if (!Step::FLAT || (et && gr > 0.0f)) {
    if (per_sample < 2) return SD_ERR_INVALID;
    const auto kernel = per_sample <= (long)CRA_THREADS * CRA_RES ? step_rescale_kernel<Step, true> : step_rescale_kernel<Step, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(CRA_THREADS), 0, stream, s, eu, et, coef, gs, gr, per_sample);
  } else if constexpr (Step::FLAT) {
    const long n = (long)batch * per_sample;
    const long nv = ((((uintptr_t)eu | (uintptr_t)et) & 15) || !s.vector_ok()) ? 0 : n / 4;
    const long work = nv > n - 4 * nv ? nv : n - 4 * nv;
    long nb = (work + 255) / 256;
    if (nb > 2048) nb = 2048;
    const auto kernel = et ? step_flat_kernel<Step, true> : step_flat_kernel<Step, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(256), 0, stream, s, eu, et, coef, gs, nv, n);
  }
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

static inline uintptr_t ptr_bits(const void* p) { return (uintptr_t)p; }

// The linear update (the epsilon- or v-prediction step of Euler / DDIM(eta = 0) / flow matching) behind the guidance rescale:
// out = coef[0] * x + coef[1] * e. x is read and out written by the same lane: out may be x. No flat kernel: without the rescale the
// step is the program executor's axpby / cfg_axpby (misc.hip), which mix the guidance with another rounding.
struct LinearStep {
  static constexpr bool FLAT = false;
  const float* x;
  float* out;
  float a, b;

  __device__ __forceinline__ void load(const float* __restrict__ c) { a = c[0], b = c[1]; }
  __device__ __forceinline__ void to_sample(long base) { x += base, out += base; }
  __device__ __forceinline__ void elem(long i, float e) const { out[i] = a * x[i] + b * e; }
};

int launch_cfg_rescale_axpby(const float* x, const float* eu, const float* et, float* out, const float* coef, float gs, float gr,
                             int batch, long per_sample, hipStream_t stream) {
  return launch_step(LinearStep{x, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One step of DPM-Solver multistep sampling (DPMSolverMultistepScheduler: dpmsolver++ / dpmsolver, orders 1 and 2) in one launch:
// the guidance combine, the guidance rescale, convert_model_output, the multistep update and the history. With coef = (p, q, A, B, D)
// in device memory, u = eu, t = et, m1 = m_prev, per element and IN THIS ORDER (tests/multistep_bounds.py derives its bound from it;
// which product fuses with which sum is the compiler's choice):
//   c   = fma(gs, t - u, u)                      (et == nullptr: c = u)
//   e   = c * k                                  (rescale form only; k of cfg_rescale_factor)
//   m0  = p * x + q * e                          -> m_out
//   out = A * x + B * m0 + D * (m0 - m1)         the difference is formed first, as the reference forms it: D carries 1 / r, and
//                                                (B + D) * m0 - D * m1 would cancel
// D == 0 (a first-order step: the first one, solver_order 1, lower_order_final / euler_at_final) is a uniform branch on the device
// value: m_prev is NOT read then -- a fresh loop's history is uninitialised, and 0 * NaN would poison the latents -- and
// out = A * x + B * m0. x / out and m_prev / m_out are read and written by the same lane at the same element, in the last pass
// only: out may be x and m_out may be m_prev (one history buffer).
struct MsCoef {
  float p, q, A, B, D;
};

__device__ __forceinline__ void multistep_elem(const MsCoef& k, bool second, float x, float e, float m1, float& o, float& m0) {
  m0 = k.p * x + k.q * e;
  o = k.A * x + k.B * m0;
  if (second) o += k.D * (m0 - m1);
}

struct MultistepStep {
  static constexpr bool FLAT = true;
  const float *x, *m_prev;
  float *out, *m_out;
  MsCoef k;
  bool second;

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(m_prev) | ptr_bits(out) | ptr_bits(m_out)) & 15); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2], c[3], c[4]};
    second = k.D != 0.0f;
  }
  __device__ __forceinline__ void to_sample(long base) { x += base, m_prev += base, out += base, m_out += base; }
  __device__ __forceinline__ void elem(long i, float e) const {
    float o, m0;
    multistep_elem(k, second, x[i], e, second ? m_prev[i] : 0.f, o, m0);
    out[i] = o;
    m_out[i] = m0;
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], ev = guided();
    f32x4 pv = {0.f, 0.f, 0.f, 0.f}, ov, mv;
    if (second) pv = reinterpret_cast<const f32x4*>(m_prev)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o, m0;
      multistep_elem(k, second, xv[j], ev[j], pv[j], o, m0);
      ov[j] = o, mv[j] = m0;
    }
    reinterpret_cast<f32x4*>(out)[i] = ov;
    reinterpret_cast<f32x4*>(m_out)[i] = mv;
  }
};

int launch_multistep_update(const float* x, const float* eu, const float* et, const float* m_prev, float* out, float* m_out,
                            const float* coef, float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(MultistepStep{x, m_prev, out, m_out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One step of UniPC sampling (UniPCMultistepScheduler: B(h) corrector then B(h) predictor, orders 1-3) in one launch: the guidance
// combine, the guidance rescale, convert_model_output, the corrector, the predictor, last_sample and the history shift. With
// coef = (p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr) in device memory (12 fp32, 16-byte aligned), L = last, h1 / h2 / h3 = the
// history planes 0 / 1 / 2 BEFORE this step's shift (plane 0 newest), per element and IN THIS ORDER (tests/unipc_bounds.py derives
// its bound from it; which product fuses with which sum is the compiler's choice, as in multistep_elem):
//   e   = the guided (and rescaled) model output, as in the multistep step
//   m_t = p * x + q * e                                                           convert_model_output on the UNCORRECTED x
//   x_c = Ac * L + Bc * h1 + C2 * (h2 - h1) + C3 * (h3 - h1) + Ct * (m_t - h1)    corr != 0; corr == 0: x_c = x         -> last
//   out = Ap * x_c + Bp * m_t + D1 * (h1 - m_t) + D2 * (h2 - m_t)
//   plane[k] <- plane[k - 1] for k = order - 1 .. 1, plane[0] <- m_t
// Every difference is formed first and then multiplied (C_k and D_k carry 1 / r_k: the regrouped form would cancel); the terms are
// summed left to right as written. A term whose coefficient is 0.0 is not formed and its operand does not enter the arithmetic: L, each
// plane inside a difference, the whole corrector at corr == 0 -- uniform branches on the device values (UpPlan), so the
// uninitialised last / hist of a fresh loop or of an img2img start never reach out (0 * NaN). A plane a term needs is also never read
// past `order`. The shift copies planes bit for bit whatever they hold. Every element of x / out, last and the planes is read and
// then written by the same lane in the last pass only: out may be x, and all pointers stay fixed from step to step.
struct UpCoef {
  float p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr;
};
struct UpPlan {   // which terms are formed, which planes are read (for a term or as the shift's source)
  bool corr, cL, cB, c2, c3, ct, d1, d2, rd1, rd2, rd3;
};

__device__ __forceinline__ UpCoef unipc_coef(const float* __restrict__ c) {
  return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11]};
}

__device__ __forceinline__ UpPlan unipc_plan(const UpCoef& k, int order) {
  UpPlan f;
  f.corr = k.corr != 0.0f;
  f.cL = f.corr && k.Ac != 0.0f;
  f.cB = f.corr && k.Bc != 0.0f;
  f.c2 = f.corr && order >= 2 && k.C2 != 0.0f;
  f.c3 = f.corr && order >= 3 && k.C3 != 0.0f;
  f.ct = f.corr && k.Ct != 0.0f;
  f.d1 = k.D1 != 0.0f;
  f.d2 = order >= 2 && k.D2 != 0.0f;
  f.rd1 = order >= 2 || f.cB || f.c2 || f.c3 || f.ct || f.d1;
  f.rd2 = order >= 3 || f.c2 || f.d2;
  f.rd3 = f.c3;
  return f;
}

__device__ __forceinline__ void unipc_elem(const UpCoef& k, const UpPlan& f, float x, float e, float L, float h1, float h2, float h3,
                                           float& o, float& xc, float& mt) {
  mt = k.p * x + k.q * e;
  xc = x;
  if (f.corr) {
    float a = 0.f;
    if (f.cL) a = k.Ac * L;
    if (f.cB) a += k.Bc * h1;
    if (f.c2) a += k.C2 * (h2 - h1);
    if (f.c3) a += k.C3 * (h3 - h1);
    if (f.ct) a += k.Ct * (mt - h1);
    xc = a;
  }
  o = k.Ap * xc + k.Bp * mt;
  if (f.d1) o += k.D1 * (h1 - mt);
  if (f.d2) o += k.D2 * (h2 - mt);
}

struct UniPCStep {
  static constexpr bool FLAT = true;
  const float* x;
  float *last, *hist;
  int order;
  long plane;   // the planes of hist are batch * per_sample elements apart, for every sample
  float* out;
  UpCoef k;
  UpPlan f;

  bool vector_ok() const {
    return !((ptr_bits(x) | ptr_bits(last) | ptr_bits(hist) | ptr_bits(out)) & 15) && !(order > 1 && (plane & 3));
  }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = unipc_coef(c);
    f = unipc_plan(k, order);
  }
  __device__ __forceinline__ void to_sample(long base) { x += base, last += base, hist += base, out += base; }
  __device__ __forceinline__ void elem(long i, float e) const {
    const float h1 = f.rd1 ? hist[i] : 0.f, h2 = f.rd2 ? hist[plane + i] : 0.f, h3 = f.rd3 ? hist[2 * plane + i] : 0.f;
    const float L = f.cL ? last[i] : 0.f;
    float o, xc, mt;
    unipc_elem(k, f, x[i], e, L, h1, h2, h3, o, xc, mt);
    out[i] = o;
    last[i] = xc;
    if (order >= 3) hist[2 * plane + i] = h2;
    if (order >= 2) hist[plane + i] = h1;
    hist[i] = mt;
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    f32x4 *l4 = reinterpret_cast<f32x4*>(last), *p0 = reinterpret_cast<f32x4*>(hist), *p1 = reinterpret_cast<f32x4*>(hist + plane),
          *p2 = reinterpret_cast<f32x4*>(hist + 2 * plane);   // (p1, p2: used below `order` only)
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f}, xv = reinterpret_cast<const f32x4*>(x)[i], ev = guided();
    f32x4 Lv = zero, h1 = zero, h2 = zero, h3 = zero, ov, cv, mv;
    if (f.cL) Lv = l4[i];
    if (f.rd1) h1 = p0[i];
    if (f.rd2) h2 = p1[i];
    if (f.rd3) h3 = p2[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o, xc, mt;
      unipc_elem(k, f, xv[j], ev[j], Lv[j], h1[j], h2[j], h3[j], o, xc, mt);
      ov[j] = o, cv[j] = xc, mv[j] = mt;
    }
    reinterpret_cast<f32x4*>(out)[i] = ov;
    l4[i] = cv;
    if (order >= 3) p2[i] = h2;
    if (order >= 2) p1[i] = h1;
    p0[i] = mv;
  }
};

int launch_unipc_update(const float* x, const float* eu, const float* et, float* last, float* hist, int order, float* out,
                        const float* coef, float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  if (order < 1 || order > 3) return SD_ERR_INVALID;
  return launch_step(UniPCStep{x, last, hist, order, (long)batch * per_sample, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One step of ancestral sampling (EulerAncestralDiscreteScheduler: a deterministic move plus fresh noise) in one launch: the guidance
// combine, the guidance rescale and prev = a x + b e + c z. With coef = (a, b, c) in device memory and z the noise plane the host
// drew, per element and IN THIS ORDER (tests/ancestral_bounds.py derives its bound from it; which product fuses with which sum is the
// compiler's choice, as in multistep_elem):
//   e   = u                                      (et == nullptr)
//       = fma(gs, t - u, u)                      (cfg_mix)
//   e   = e * k                                  (rescale form only; k of cfg_rescale_factor)
//   out = a * x + b * e
//   out = out + c * z                            only if c != 0
// c == 0 (the last row of every schedule: sigma_up = 0) is a uniform branch on the device value: noise is NOT read then, so a stale or
// NaN plane cannot reach the final latents (0 * NaN), and a caller that knows the row may pass a null noise. x is read and out written
// by the same lane at the same element, in the last pass only: out may be x.
struct AnCoef {
  float a, b, c;
};

__device__ __forceinline__ float ancestral_elem(const AnCoef& k, bool noisy, float x, float e, float z) {
  float o = k.a * x + k.b * e;
  if (noisy) o += k.c * z;
  return o;
}

struct AncestralStep {
  static constexpr bool FLAT = true;
  const float *x, *noise;
  float* out;
  AnCoef k;
  bool noisy;

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(noise) | ptr_bits(out)) & 15); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2]};
    noisy = k.c != 0.0f;
  }
  __device__ __forceinline__ void to_sample(long base) {
    x += base, out += base;
    if (noisy) noise += base;   // (never formed from a null pointer)
  }
  __device__ __forceinline__ void elem(long i, float e) const { out[i] = ancestral_elem(k, noisy, x[i], e, noisy ? noise[i] : 0.f); }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], ev = guided();
    f32x4 zv = {0.f, 0.f, 0.f, 0.f}, ov;
    if (noisy) zv = reinterpret_cast<const f32x4*>(noise)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = ancestral_elem(k, noisy, xv[j], ev[j], zv[j]);
    reinterpret_cast<f32x4*>(out)[i] = ov;
  }
};

int launch_ancestral_update(const float* x, const float* eu, const float* et, const float* noise, float* out, const float* coef,
                            float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(AncestralStep{x, noise, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One model evaluation of a two-stage, second-order step (HeunDiscreteScheduler: an Euler step, then Heun's correction from the same
// start) in one launch: the guidance combine, the guidance rescale, the derivative and the update. The step's state lives in two
// caller-owned planes: S (the sample the step started from) and D (the derivative there). With coef = (p, q, h, g, second) in device
// memory, per element and IN THIS ORDER (tests/heun_bounds.py derives its bound from it; which product fuses with which sum is the
// compiler's choice, as in multistep_elem):
//   e   = the guided (and rescaled) model output, as in the ancestral step
//   d   = p * x + q * e                          p == 0 (epsilon prediction): d = q * e, the product with x is not formed
//   second == 0 (stage 1):  out = x + h * d      S <- x (bit copy), D <- d; S and D are NOT read
//   second != 0 (stage 2):  m   = g * D + d      g == 0: m = d and D is NOT read; g == 1 (Heun): the product is exact
//                           out = S + h * m      S and D are NOT written
// second, p == 0 and g == 0 are uniform branches on the device values, set once in load(): one captured node replays both stages with
// only the row changing. State a stage does not need never enters the arithmetic -- the S / D of a fresh loop are uninitialised, and
// 0 * NaN would poison the latents; stage 2 at p == 0 does not read x either. g weights the parked derivative: Heun's average takes
// 1 (h carries the 1 / 2); a midpoint method (KDPM2) would take 0 and never read D. x is read and out written by the same lane in the
// last pass only: out may be x. S and D are touched by that same lane at the same element; they overlap nothing else.
struct HeCoef {
  float p, q, h, g, second;
};

__device__ __forceinline__ void heun_elem(const HeCoef& k, bool second, bool px, bool gd, float x, float e, float S, float D, float& o,
                                          float& d) {
  d = px ? k.p * x + k.q * e : k.q * e;
  if (!second) {
    o = x + k.h * d;
  } else {
    const float m = gd ? k.g * D + d : d;
    o = S + k.h * m;
  }
}

struct HeunStep {
  static constexpr bool FLAT = true;
  const float* x;
  float *sample, *deriv, *out;
  HeCoef k;
  bool second, px, gd, rx;   // stage 2; p != 0; stage 2 reads D; x is read (stage 1, or p != 0)

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(sample) | ptr_bits(deriv) | ptr_bits(out)) & 15); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2], c[3], c[4]};
    second = k.second != 0.0f;
    px = k.p != 0.0f;
    gd = second && k.g != 0.0f;
    rx = !second || px;
  }
  __device__ __forceinline__ void to_sample(long base) { x += base, sample += base, deriv += base, out += base; }
  __device__ __forceinline__ void elem(long i, float e) const {
    const float xv = rx ? x[i] : 0.f;
    float o, d;
    heun_elem(k, second, px, gd, xv, e, second ? sample[i] : 0.f, gd ? deriv[i] : 0.f, o, d);
    out[i] = o;
    if (!second) {
      sample[i] = xv;
      deriv[i] = d;
    }
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    f32x4 *s4 = reinterpret_cast<f32x4*>(sample), *d4 = reinterpret_cast<f32x4*>(deriv);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 xv = zero, Sv = zero, Dv = zero, ov, dv;
    if (rx) xv = reinterpret_cast<const f32x4*>(x)[i];
    const f32x4 ev = guided();
    if (second) Sv = s4[i];
    if (gd) Dv = d4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o, d;
      heun_elem(k, second, px, gd, xv[j], ev[j], Sv[j], Dv[j], o, d);
      ov[j] = o, dv[j] = d;
    }
    reinterpret_cast<f32x4*>(out)[i] = ov;
    if (!second) {
      s4[i] = xv;
      d4[i] = dv;
    }
  }
};

int launch_heun_update(const float* x, const float* eu, const float* et, float* sample, float* deriv, float* out, const float* coef,
                       float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(HeunStep{x, sample, deriv, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One model evaluation of a two-stage midpoint step (KDPM2DiscreteScheduler, "DPM2": an Euler step to the midpoint sigma, then the
// whole step from the same start with the derivative found there; KDPM2AncestralDiscreteScheduler, "DPM2 a": the same, ending lower
// and adding fresh noise) in one launch: the guidance combine, the guidance rescale, the derivative and the update. The step's state
// is ONE caller-owned plane, S (the sample the step started from): a midpoint method never reads the first derivative again, so
// stage 1 writes a plane fewer than HeunStep. With coef = (p, q, h, c, second) in device memory and z the noise plane the host drew,
// per element and IN THIS ORDER (tests/dpm2_bounds.py derives its bound from it; which product fuses with which sum is the compiler's
// choice, as in multistep_elem):
//   e   = the guided (and rescaled) model output, as in the ancestral step
//   d   = p * x + q * e                          p == 0 (epsilon prediction): d = q * e, the product with x is not formed
//   second == 0 (stage 1):  out = x + h * d      S <- x (bit copy); S and noise are NOT read
//   second != 0 (stage 2):  out = S + h * d      S is NOT written
//                           out = out + c * z    only if c != 0 (DPM2 a); c == 0: noise is NOT read
// second, p == 0 and c == 0 are uniform branches on the device values, set once in load(): one captured node replays both stages with
// only the row changing. State a stage does not need never enters the arithmetic -- the S of a fresh loop is uninitialised, a noise
// plane may be stale or null where c == 0, and 0 * NaN would poison the latents; stage 2 at p == 0 does not read x either. The noise
// counts in stage 2 only: a stage-1 row never reads it, whatever its c. x is read and out written by the same lane in the last pass
// only: out may be x. S is touched by that same lane at the same element; it overlaps nothing else.
struct MpCoef {
  float p, q, h, c, second;
};

__device__ __forceinline__ float midpoint_elem(const MpCoef& k, bool second, bool px, bool noisy, float x, float e, float S, float z) {
  const float d = px ? k.p * x + k.q * e : k.q * e;
  float o = (second ? S : x) + k.h * d;
  if (noisy) o += k.c * z;
  return o;
}

struct MidpointStep {
  static constexpr bool FLAT = true;
  const float *x, *noise;
  float *sample, *out;
  MpCoef k;
  bool second, px, noisy, rx;   // stage 2; p != 0; stage 2 adds c z; x is read (stage 1, or p != 0)

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(noise) | ptr_bits(sample) | ptr_bits(out)) & 15); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2], c[3], c[4]};
    second = k.second != 0.0f;
    px = k.p != 0.0f;
    noisy = second && k.c != 0.0f;
    rx = !second || px;
  }
  __device__ __forceinline__ void to_sample(long base) {
    x += base, sample += base, out += base;
    if (noisy) noise += base;   // (never formed from a null pointer)
  }
  __device__ __forceinline__ void elem(long i, float e) const {
    const float xv = rx ? x[i] : 0.f;
    out[i] = midpoint_elem(k, second, px, noisy, xv, e, second ? sample[i] : 0.f, noisy ? noise[i] : 0.f);
    if (!second) sample[i] = xv;
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    f32x4* s4 = reinterpret_cast<f32x4*>(sample);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 xv = zero, Sv = zero, zv = zero, ov;
    if (rx) xv = reinterpret_cast<const f32x4*>(x)[i];
    const f32x4 ev = guided();
    if (second) Sv = s4[i];
    if (noisy) zv = reinterpret_cast<const f32x4*>(noise)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = midpoint_elem(k, second, px, noisy, xv[j], ev[j], Sv[j], zv[j]);
    reinterpret_cast<f32x4*>(out)[i] = ov;
    if (!second) s4[i] = xv;
  }
};

int launch_dpm2_update(const float* x, const float* eu, const float* et, const float* noise, float* sample, float* out,
                       const float* coef, float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(MidpointStep{x, noise, sample, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One model evaluation of PLMS sampling (PNDMScheduler with skip_prk_steps: a linear multistep method over up to four model outputs,
// whose second evaluation averages two outputs and steps again from the first sample) in one launch: the guidance combine, the
// guidance rescale, the history combination, _get_prev_sample, the history and the parked sample. The state lives in caller-owned
// planes: P (`park`, the sample the loop started from) and a RING of three planes (`hist`, batch * per_sample elements apart) with
// the last three guided outputs. With coef = (a, b, p, q, w0, w1, w2, w3, slot, park, from_park, 0) in device memory (12 fp32: the
// row is padded to 48 bytes), h1 / h2 / h3 the ring planes slot - 1 / slot - 2 / slot - 3 mod 3, per element and IN THIS ORDER
// (tests/plms_bounds.py derives its bound from it; which product fuses with which sum is the compiler's choice, as in multistep_elem):
//   e   = the guided (and rescaled) model output, as in the ancestral step
//   m   = w0 * e
//   m   = m + w1 * h1                            only if w1 != 0; likewise w2 * h2, then w3 * h3: a plane is read for its term only
//   S   = from_park != 0 ? P : x                 from_park: x is NOT read; otherwise P is NOT read
//   m   = p * S + q * m                          only if p != 0 (v-prediction); epsilon: the product with S is not formed
//   out = a * S + b * m
//   plane[slot] <- e                             unless from_park: the UNCONVERTED guided (and rescaled) output
//   P   <- x (bit copy)                          only if park != 0 (and not from_park)
// The oldest plane, slot - 3 = slot mod 3, is the one e replaces: the same lane reads it (for w3) at the same element before it writes
// e there, so the ring advances by the row's slot alone and no plane is ever copied. slot is 0, 1 or 2; any other device value is
// taken as the nearest of them (NaN: 0), so that a wrong row cannot index outside hist. All flags, every weight != 0 and p != 0 are
// uniform branches on the device values, set once in load(): one captured node replays every evaluation of a loop with only the row
// changing and every pointer fixed. State an evaluation does not need never enters the arithmetic -- a fresh loop's ring and P are
// uninitialised, and 0 * NaN would poison the latents. S is read and out written by the same lane in the last pass only: out may be x.
// P and the ring are touched by that same lane at the same element; they overlap nothing else.
struct PlCoef {
  float a, b, p, q, w0, w1, w2, w3, slot, park, from_park;
};

__device__ __forceinline__ float plms_elem(const PlCoef& k, bool r1, bool r2, bool r3, bool px, float S, float e, float h1, float h2,
                                           float h3) {
  float m = k.w0 * e;
  if (r1) m += k.w1 * h1;
  if (r2) m += k.w2 * h2;
  if (r3) m += k.w3 * h3;
  if (px) m = k.p * S + k.q * m;
  return k.a * S + k.b * m;
}

struct PlmsStep {
  static constexpr bool FLAT = true;
  const float* x;
  float *park, *hist;
  long plane;   // the planes of hist are batch * per_sample elements apart, for every sample
  float* out;
  PlCoef k;
  float *h1, *h2, *h3;          // the ring planes slot - 1, slot - 2 and slot (= slot - 3: the oldest, and where e goes)
  bool fp, pk, px, r1, r2, r3;   // S = P; P <- x; p != 0; the planes that are read

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(park) | ptr_bits(hist) | ptr_bits(out)) & 15) && !(plane & 3); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10]};
    const int s = k.slot >= 1.5f ? 2 : k.slot >= 0.5f ? 1 : 0;
    h1 = hist + (s == 0 ? 2 : s - 1) * plane;
    h2 = hist + (s == 2 ? 0 : s + 1) * plane;
    h3 = hist + s * plane;
    fp = k.from_park != 0.0f;
    pk = !fp && k.park != 0.0f;
    px = k.p != 0.0f;
    r1 = k.w1 != 0.0f, r2 = k.w2 != 0.0f, r3 = k.w3 != 0.0f;
  }
  __device__ __forceinline__ void to_sample(long base) { x += base, park += base, h1 += base, h2 += base, h3 += base, out += base; }
  __device__ __forceinline__ void elem(long i, float e) const {
    const float S = fp ? park[i] : x[i];
    out[i] = plms_elem(k, r1, r2, r3, px, S, e, r1 ? h1[i] : 0.f, r2 ? h2[i] : 0.f, r3 ? h3[i] : 0.f);
    if (!fp) h3[i] = e;
    if (pk) park[i] = S;
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    f32x4 *p4 = reinterpret_cast<f32x4*>(park), *w4 = reinterpret_cast<f32x4*>(h3);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 Sv = fp ? p4[i] : reinterpret_cast<const f32x4*>(x)[i], ev = guided();
    f32x4 v1 = zero, v2 = zero, v3 = zero, ov;
    if (r1) v1 = reinterpret_cast<const f32x4*>(h1)[i];
    if (r2) v2 = reinterpret_cast<const f32x4*>(h2)[i];
    if (r3) v3 = w4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = plms_elem(k, r1, r2, r3, px, Sv[j], ev[j], v1[j], v2[j], v3[j]);
    reinterpret_cast<f32x4*>(out)[i] = ov;
    if (!fp) w4[i] = ev;
    if (pk) p4[i] = Sv;
  }
};

int launch_plms_update(const float* x, const float* eu, const float* et, float* park, float* hist, float* out, const float* coef,
                       float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(PlmsStep{x, park, hist, (long)batch * per_sample, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

// One model evaluation of DPM-Solver SINGLESTEP sampling (DPMSolverSinglestepScheduler: dpmsolver++ / dpmsolver, orders 1-3, midpoint /
// heun; an order-k evaluation does not step from the current latents but from the sample parked k - 1 evaluations earlier, with the
// converted outputs of its group as differences against the group's first) in one launch: the guidance combine, the guidance
// rescale, convert_model_output, the update, the parked sample and the group's outputs. The state lives in caller-owned planes: S
// (`park`, the sample the group started from) and TWO planes of `hist`, batch * per_sample elements apart: plane 0 the group's first
// converted output, plane 1 its second. A group is an order-1 evaluation followed by an order-2 and then an order-3 one, as far as it
// goes, so each plane has one writer per group and a fixed meaning: nothing is shifted and no plane is copied. With coef =
// (p, q, A, B, E1, E2, order, keep) in device memory (8 fp32: 32 bytes), per element and IN THIS ORDER (tests/singlestep_bounds.py
// derives its bound from it; which product fuses with which sum is the compiler's choice, as in multistep_elem):
//   e   = the guided (and rescaled) model output, as in the ancestral step
//   m0  = p * x + q * e
//   order 1:  out = A * x + B * m0                        S <- x (bit copy), plane 0 <- m0; S and hist are NOT read
//   order 2:  b   = plane 0
//             out = A * S + B * b + E1 * (m0 - b)         plane 1 <- m0 only if keep != 0 (an order-3 evaluation follows); S and
//                                                         plane 0 are NOT written
//   order 3:  b   = plane 0, m1 = plane 1
//             out = A * S + B * b + E1 * (m0 - b)
//             out = out + E2 * (m1 - b)                   only if E2 != 0 (heun); E2 == 0 (midpoint): plane 1 is NOT read
//                                                         nothing but out is written
// Every difference is taken against b and formed before it is multiplied: E1 and E2 carry 1 / r0, 1 / r1 and 1 / (r0 - r1), and the
// regrouped (B - E1 - E2) * b + E1 * m0 + E2 * m1 would cancel, as in multistep_elem. order, keep and E2 != 0 are uniform branches on
// the device values, set once in load(): one captured node replays every evaluation of a loop with only the row changing and every
// pointer fixed. order is 1, 2 or 3; any other device value is taken as the nearest of them (NaN: 1), so that a wrong row cannot do
// anything the three branches don't. State an evaluation does not need never enters the arithmetic -- a fresh loop's S and hist are
// uninitialised, and 0 * NaN would poison the latents. x is read by every row (for m0) and out written by the same lane in the last
// pass only: out may be x. S and hist are touched by that same lane at the same element; they overlap nothing else.
struct SsCoef {
  float p, q, A, B, E1, E2, order, keep;
};

__device__ __forceinline__ void singlestep_elem(const SsCoef& k, int order, bool heun, float x, float e, float S, float b, float m1,
                                                float& o, float& m0) {
  m0 = k.p * x + k.q * e;
  if (order == 1) {
    o = k.A * x + k.B * m0;
  } else {
    o = k.A * S + k.B * b + k.E1 * (m0 - b);
    if (heun) o += k.E2 * (m1 - b);
  }
}

struct SinglestepStep {
  static constexpr bool FLAT = true;
  const float* x;
  float *park, *hist;
  long plane;   // the planes of hist are batch * per_sample elements apart, for every sample
  float* out;
  SsCoef k;
  int order;
  bool keep, heun;   // order 2 writes plane 1; order 3 adds E2 (m1 - b)

  bool vector_ok() const { return !((ptr_bits(x) | ptr_bits(park) | ptr_bits(hist) | ptr_bits(out)) & 15) && !(plane & 3); }
  __device__ __forceinline__ void load(const float* __restrict__ c) {
    k = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
    order = k.order >= 2.5f ? 3 : k.order >= 1.5f ? 2 : 1;
    keep = order == 2 && k.keep != 0.0f;
    heun = order == 3 && k.E2 != 0.0f;
  }
  __device__ __forceinline__ void to_sample(long base) { x += base, park += base, hist += base, out += base; }
  __device__ __forceinline__ void elem(long i, float e) const {
    const float xv = x[i];
    const float S = order > 1 ? park[i] : 0.f, b = order > 1 ? hist[i] : 0.f, m1 = heun ? hist[plane + i] : 0.f;
    float o, m0;
    singlestep_elem(k, order, heun, xv, e, S, b, m1, o, m0);
    out[i] = o;
    if (order == 1) {
      park[i] = xv;
      hist[i] = m0;
    } else if (keep) {
      hist[plane + i] = m0;
    }
  }
  template <class E>
  __device__ __forceinline__ void vec(long i, E&& guided) const {
    f32x4 *s4 = reinterpret_cast<f32x4*>(park), *p0 = reinterpret_cast<f32x4*>(hist), *p1 = reinterpret_cast<f32x4*>(hist + plane);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f}, xv = reinterpret_cast<const f32x4*>(x)[i], ev = guided();
    f32x4 Sv = zero, bv = zero, m1 = zero, ov, mv;
    if (order > 1) {
      Sv = s4[i];
      bv = p0[i];
    }
    if (heun) m1 = p1[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o, m0;
      singlestep_elem(k, order, heun, xv[j], ev[j], Sv[j], bv[j], m1[j], o, m0);
      ov[j] = o, mv[j] = m0;
    }
    reinterpret_cast<f32x4*>(out)[i] = ov;
    if (order == 1) {
      s4[i] = xv;
      p0[i] = mv;
    } else if (keep) {
      p1[i] = mv;
    }
  }
};

int launch_singlestep_update(const float* x, const float* eu, const float* et, float* park, float* hist, float* out, const float* coef,
                             float gs, float gr, int batch, long per_sample, hipStream_t stream) {
  return launch_step(SinglestepStep{x, park, hist, (long)batch * per_sample, out}, eu, et, coef, gs, gr, batch, per_sample, stream);
}

}  // namespace sd
