"""Float64 reference and elementwise bound for mi355x_sd_multistep_update (csrc/misc.hip multistep_kernel / multistep_rescale_kernel):
one step of DPM-Solver multistep sampling -- guidance combine, guidance rescale, convert_model_output, the update and its history --
in one launch. The sibling of tests/guidance_bounds.py, whose constants, statistics bound (_ss, chain, K_R) and check() it imports:
|out - ref| <= 2 u |ref| + e for an fp32 store, u = 2^-24, over EVERY element of both outputs.

What the kernel computes per element, in this order (coef = (p, q, A, B, D) fp32, t = eps_text, u = eps_uncond, m1 = m_prev):
    c   = fma(gs, fl(t - u), u)                        (no eps_text: c = u, exactly)
    E   = fl(c * k)                                    guidance_rescale > 0 only; k of guidance_bounds (per sample, same tree sums)
    m0  = fl(fl(p x) + fl(q E))                        -> m_out
    out = fl(fl(fl(A x) + fl(B m0)) + fl(D fl(m0 - m1)))          D == 0: out = fl(fl(A x) + fl(B m0)) and m1 is NOT read
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (gamma(k) = k u / (1 - k u); 1.01 absorbs second-order products of u terms, as in guidance_bounds):
  * c, k: e_c = u (3 |gs| |t - u| + |u|) and e_k exactly as guidance_bounds derives them; without eps_text e_c = 0, at gr = 0 k = 1, e_k = 0.
  * E = c k, one rounded product of computed factors: e_E = (|c| + e_c)(|k| + e_k) - |c| |k| + 1.01 u (|c| + e_c)(|k| + e_k).
  * m0, two products and a sum of a read value and a computed one: e_m0 = |q| e_E + 2 u (|p x| + |q| (|E| + e_E)). This is m_out's bound.
  * the three-term sum. m1 is read, not computed. The computed m0 enters through B and, in the difference, through D:
    (|B| + |D|) e_m0. The roundings: A x, B m0, their sum; the difference, its product with D, the last sum -- no term passes
    through more than three:  e_out = (|B| + |D|) e_m0 + 1.01 * 3 u (|A x| + |B| (|m0| + e_m0) + |D| (|m0 - m1| + e_m0)).
    The regrouped (B + D) m0 - D m1 would carry u (|B + D| |m0| + |D| |m1|) instead of u |D| |m0 - m1|: with D ~ 1 / r large and
    m0 ~ m1 it leaves the bound (tests/test_multistep_bounds.py injects it).

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs the
fused loop saw. Two errors travel: E_x of the latents and E_m of the history. With (p, q, A, B, D) the float64 coefficients, x32 the
fp32 table entries, x_i / h_i the fused loop's latents / history, ref the kernel's float64 value at the fused inputs:
    dm0     = |p| E_x + |p32 - p| |x_i| + |q32 - q| |E|                                  (ref m0 against the generic m0)
    E_x'    = |A| E_x + |A32 - A| |x_i| + (|B| + |D|) dm0 + |B32 - B| |m0| + |D| E_m + |D32 - D| |m0 - h_i| + (2 u |ref| + e_out)
    E_m'    = dm0 + (2 u |m0| + e_m0)
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (DPM-Solver: 1), E_m starts at 0 and is not used while D = 0.
"""
import torch

from paddlemix_amd.schedulers import DPMSolverMultistepScheduler
from tests.guidance_bounds import K_R, RESIDENT, _ss, chain
from tests.norm_bounds import fp32
from tests.rowmap_bounds import U32
from tests.step_pieces import base_inputs

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def schedule_rows(steps=20, **kw):
    """(p, q, A, B, D) of every step of a dpmsolver++ midpoint schedule, as Python floats"""
    sch = DPMSolverMultistepScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    return [sch.multistep_coefficients(t) for t in sch.timesteps]


ROWS = schedule_rows()
MID, FIRST = ROWS[10], ROWS[0]    # a second-order step at mid schedule (D != 0) and the first step (D = 0)
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0.7, row MID, CFG, random inputs
    "b1 n1 gr0": dict(batch=1, n=1, gr=0.0),
    "b1 n2 smallest rescale": dict(batch=1, n=2),
    "b1 n252 below one block": dict(batch=1, n=252),
    "b1 n252 gr0": dict(batch=1, n=252, gr=0.0),
    "b3 n4092 gr0 vectors": dict(batch=3, n=4092, gr=0.0),
    "b3 n4093 gr0 vectors + tail": dict(batch=3, n=4093, gr=0.0),
    "b3 n4092 gr0 x offset one element": dict(batch=3, n=4092, gr=0.0, misalign=True),
    "b3 n4093 odd rescale": dict(batch=3, n=4093),
    "b2 n4096 exact": dict(batch=2, n=4096),
    "b2 n32772 loop form": dict(batch=2, n=RESIDENT + 4),
    "b2 n4092 offset 64": dict(batch=2, n=4092, kind="offset"),
    "b3 n4093 no eps_text": dict(batch=3, n=4093, cfg=False),
    "b2 n4096 no eps_text": dict(batch=2, n=4096, cfg=False),
    "b2 n4096 gr0": dict(batch=2, n=4096, gr=0.0),
    "b2 n4096 gr0 D0 NaN history": dict(batch=2, n=4096, gr=0.0, row="first", nan_history=True),
    "b2 n4093 D0 NaN history": dict(batch=2, n=4093, row="first", nan_history=True),
    "b2 n4096 gr0 out=x m_out=m_prev": dict(batch=2, n=4096, gr=0.0, alias=True),
    "b2 n4096 out=x m_out=m_prev": dict(batch=2, n=4096, alias=True),
    "b2 n32772 out=x m_out=m_prev": dict(batch=2, n=RESIDENT + 4, alias=True),
    "b8 n65536 workload": dict(batch=8, n=4 * 128 * 128),
    "b8 n65536 gr0 workload": dict(batch=8, n=4 * 128 * 128, gr=0.0),
}


def inputs(name):
    """dict(x, eu, et (None: no guidance), m1, coef, gs, gr) of a case: CPU fp32 [batch, n], seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    m1 = 2.0 * torch.randn(shape, generator=g)
    if s.get("nan_history"):
        m1 = torch.full(shape, float("nan"))
    row = FIRST if s.get("row") == "first" else MID
    return dict(x=x, eu=eu, et=et, m1=m1, coef=torch.tensor(row, dtype=torch.float32),
                gs=s.get("gs", 7.5), gr=s.get("gr", 0.7))


def guided(eu, et, gs, gr, depth=None):
    """the guided (and rescaled) model output E the update sees, float64, and the bound e_E on the kernel's computed value"""
    u = eu.double()
    if et is None:
        return u, torch.zeros_like(u)
    gs, gr = fp32(gs), fp32(gr)
    t = et.double()
    d = t - u
    c = u + gs * d
    e_c = U32 * (3 * abs(gs) * d.abs() + u.abs())
    if gr == 0.0:
        return c, e_c
    L = chain(u.shape[1]) if depth is None else depth
    SSt, Et = _ss(t, torch.zeros_like(t), L)
    SSc, Ec = _ss(c, e_c, L)
    r = (SSt / SSc).sqrt()
    rho_t, rho_c = Et / SSt, Ec / SSc
    up = torch.where(rho_c < 1, ((1 + rho_t) / (1 - rho_c).clamp_min(1e-300)).sqrt(), torch.full_like(rho_c, float("inf")))
    dr = up * (1 + 1.01 * K_R * U32) - 1
    k = gr * r + (1 - gr)
    e_k = abs(gr) * r * dr + 1.01 * 2 * U32 * (abs(gr) * r * (1 + dr) + abs(1 - gr))
    big = (c.abs() + e_c) * (k.abs() + e_k)
    return c * k, big - c.abs() * k.abs() + 1.01 * U32 * big


def multistep_update(x, eu, et, m1, coef, gs, gr, depth=None):
    """x, eu, et (or None), m1 fp32 [batch, n]; coef fp32 (p, q, A, B, D); gs, gr as the C ABI passes them ->
    dict(out, e_out, m0, e_m0, E) float64 [batch, n]"""
    p, q, A, B, D = coef.double().tolist()
    E, e_E = guided(eu, et, gs, gr, depth)
    px, Ax = p * x.double(), A * x.double()
    m0 = px + q * E
    e_m0 = abs(q) * e_E + 2 * U32 * (px.abs() + abs(q) * (E.abs() + e_E))
    out = Ax + B * m0
    diff = torch.zeros_like(m0)
    if D != 0.0:
        diff = m0 - m1.double()
        out = out + D * diff
    e_out = (abs(B) + abs(D)) * e_m0 + 1.01 * 3 * U32 * (Ax.abs() + abs(B) * (m0.abs() + e_m0) + abs(D) * (diff.abs() + e_m0))
    return dict(out=out, e_out=e_out, m0=m0, e_m0=e_m0, E=E, diff=diff)


def accumulated(xs, hs, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every step of a loop whose model outputs were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before step i; hs[i]: its history buffer before step i (anything at i = 0);
    outs[i]: its fp32 model output ([2 B, ...] = [uncond, text] with cfg); coef64: (p, q, A, B, D) per step as Python floats
    -> list of float64 bounds shaped like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    E_m = torch.zeros_like(E_x)
    res = []
    for x, h, o, c64 in zip(xs, hs, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        xf = x.flatten(1)
        r = multistep_update(xf, o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, h.flatten(1), c32, gs, gr if cfg else 0.0)
        p, q, A, B, D = c64
        dp, dq, dA, dB, dD = (abs(a - b) for a, b in zip(c32.double().tolist(), c64))
        dm0 = abs(p) * E_x + dp * xf.double().abs() + dq * r["E"].abs()
        E_x = abs(A) * E_x + dA * xf.double().abs() + (abs(B) + abs(D)) * dm0 + dB * r["m0"].abs() + dD * r["diff"].abs() \
            + (abs(D) * E_m if D != 0.0 else 0.0) + 2 * U32 * r["out"].abs() + r["e_out"]
        E_m = dm0 + 2 * U32 * r["m0"].abs() + r["e_m0"]
        res.append(E_x.reshape(x.shape))
    return res


def generic_loop(sch, timesteps, x0, outs, gs, gr, cfg=True):
    """The generic loop's lines (pipeline.py: chunk, guidance combine, rescale_noise_cfg, scheduler.step) in float64 over
    ``timesteps`` on recorded model outputs: where the pipeline's own generic loop cannot run in float64 (img2img casts its start
    to fp32). The scheduler must be as set_timesteps left it."""
    from paddlemix_amd.pipeline import rescale_noise_cfg
    x = x0.double()
    for t, o in zip(timesteps, outs):
        e = o.double()
        if cfg:
            eu, et = e.chunk(2)
            e = eu + gs * (et - eu)
            if gr > 0.0:
                e = rescale_noise_cfg(e, et, gr)
        x = sch.step(e, t, x, return_dict=False)[0]
    return x
