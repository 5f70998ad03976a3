"""Float64 reference and elementwise bound for mi355x_sd_cfg_rescale_axpby (csrc/misc.hip cfg_rescale_axpby_kernel): the guidance
combine, the guidance rescale (rescale_noise_cfg of paddlemix_amd/pipeline.py) and the linear scheduler update in one launch. The
sibling of tests/rowmap_bounds.py, with its constants (imported, not restated) and its check(): |out - ref| <= 2 u |ref| + e for
an fp32 store, u = u32 = 2^-24, over EVERY element. Plain Python + torch; runs on whatever device the tensors live on.

What the kernel computes, per sample of n = per_sample elements (t = eps_text, u = eps_uncond, all fp32):
    c_i = fma(gs, fl(t_i - u_i), u_i)                       the guidance combine
    m_v = fl(S_v * fl(1 / fl(n))),  S_v = tree sum of v     v = t and v = c
    Q_v = tree sum of fl(fl(v_i - m_v)^2)                   the second pass: deviations from the computed mean
    s_v = sqrt(fl(Q_v * fl(1 / fl(n - 1)))),  r = fl(s_t / s_c)
    k   = fl(fl(gr * r) + fl(1 - gr))
    out = fl(a x_i + fl(b * fl(c_i * k)))                   (which products fuse is the compiler's choice)
A tree sum: a lane adds its elements tid, tid + 1024, ... in order (ceil(n / 1024) terms, the first onto 0: exact), a 64-lane
butterfly (6 levels), a 16-partial butterfly (4 levels): no term passes through more than L = ceil(n / 1024) + 10 additions.

The bound, from the arithmetic alone (gamma(k) = k u / (1 - k u)):
  * c: as in rowmap_bounds.cfg_axpby, e_c = u (3 |gs| |t - u| + |u|); it covers the fused and the unfused form. t is read, not
    computed: e_t = 0.
  * the mean of computed values v'_i = v_i + eps_i, |eps_i| <= e_i: the tree sum is off by at most sum e_i + gamma(L) sum (|v_i| + e_i);
    fl(n) (exact below 2^24, else u), the reciprocal (correctly rounded or v_rcp_f32: 2 u) and the product (u) add 4 u |m|:
        dm = (1 + 4 u) (sum e_i + gamma(L) sum (|v_i| + e_i)) / n + 4 u |m|.
  * the sum of squares. With D_i = v_i - m the exact deviations (sum D_i = 0, SS = sum D_i^2) and Delta = m' - m, |Delta| <= dm:
        sum (v'_i - m')^2 = SS + 2 sum D_i eps_i - 2 Delta sum D_i + sum (eps_i - Delta)^2,
    and the third term vanishes: THIS is the condition number of the two-pass form -- the error of the mean enters squared, dm^2 / var
    relatively, however large the offset m is. (The one-pass form sum v^2 - n m^2 carries gamma(L) sum v^2 instead: (m / sigma)^2
    times more; tests/test_guidance_bounds.py injects it.) So in exact arithmetic the second pass is off by at most
        A = 2 sum |D_i| e_i + sum (e_i + dm)^2,
    and its own roundings -- the subtraction, the square, the chain, every term positive -- are relative: gamma(L + 3) (SS + A):
        E_SS = A + gamma(L + 3) (SS + A),  rho = E_SS / SS.
  * r = s_t / s_c: the square root halves a relative error; fl(n - 1), its reciprocal and the product (4 u, halved: 2 u), the square
    root (<= 1 ulp: 2 u) for each of the two, and the division (2 u): K_R = 10 u on top of
        r' / r <= sqrt((1 + rho_t) / (1 - rho_c)),   dr = sqrt((1 + rho_t) / (1 - rho_c)) (1 + 1.01 K_R u) - 1
    (the lower side sqrt((1 - rho_t) / (1 + rho_c)) is closer to 1). rho_c >= 1 -- a variance the roundings of c alone could
    cancel -- has no bound (inf): such an input is not a test case. Neither is a variance of exactly zero: the kernel divides as
    the reference does.
  * k = gr r + (1 - gr): e_k = |gr| r dr + 1.01 * 2 u (|gr| r (1 + dr) + |1 - gr|)    (1 - gr, the product, the sum).
    At gr = 0 this is 0: k = fl(0 * r + 1) = 1 exactly, and the whole bound falls back to cfg_axpby's.
  * P = b c k, two rounded products of computed factors: e_P = |b| ((|c| + e_c) (|k| + e_k) - |c| |k|) + 1.01 * 2 u |b| (|c| + e_c) (|k| + e_k);
    out = a x + P as in axpby: e = e_P + 2 u (|a x| + |P| + e_P).
The 1.01 factors absorb the second-order products of the u terms (as in rowmap_bounds.softmax).

accumulated() carries that bound through a denoising loop: tests drive the generic loop (fused_update=False) in float64 with the
model outputs the fused loop saw, so the only differences are the kernel's deviation from its float64 value, the fp32 rounding of
the (a, b) table, and what the earlier steps left, which the update multiplies by |a|:
    E_0 = u |x_0| (the fp32 product with init_noise_sigma),   E_{i+1} = |a_i| E_i + (2 u |ref_i| + e_i) + |a32 - a| |x_i| + |b32 - b| |c k|.
"""
import torch

from tests.norm_bounds import RCP, fp32, gamma
from tests.rowmap_bounds import U32
from tests.step_pieces import base_inputs

THREADS, RES = 1024, 32          # csrc/misc.hip CRA_THREADS, CRA_RES: block size, register-resident values per lane and array
RESIDENT = THREADS * RES         # the largest sample that is read once; above it the kernel loops and re-reads
K_R = 4 + 4 + RCP / U32          # roundings between the two sums of squares and r, in units of u (see above)
COEF = (0.9873, -0.4127)         # a v-prediction Euler step's (a, b) at mid schedule
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0.7, random inputs
    "b1 n252 below one block": dict(batch=1, n=4 * 9 * 7),
    "b3 n4092 ragged": dict(batch=3, n=4 * 33 * 31),
    "b3 n4093 odd": dict(batch=3, n=4 * 33 * 31 + 1),
    "b1 n2 smallest": dict(batch=1, n=2),
    "b2 n4096 exact": dict(batch=2, n=16 * 16 * 16),
    "b2 n32772 loop form": dict(batch=2, n=RESIDENT + 4),
    "b2 n4092 offset 64": dict(batch=2, n=4092, kind="offset"),
    "b2 n4096 gr0": dict(batch=2, n=4096, gr=0.0),
    "b2 n4096 gr1 gs1": dict(batch=2, n=4096, gr=1.0, gs=1.0),
    "b2 n4096 out=x": dict(batch=2, n=4096, alias=True),
    "b8 n65536 workload": dict(batch=8, n=4 * 128 * 128),
}


def inputs(name):
    """(x, eu, et, coef, gs, gr) of a case: CPU fp32 [batch, n], seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    return x, eu, et, torch.tensor(COEF), s.get("gs", 7.5), s.get("gr", 0.7)


def chain(n):
    return (n + THREADS - 1) // THREADS + 6 + 4


def _ss(v, e, L):
    """v float64 [batch, n] exact values, e their computed versions' error bounds -> (SS, E_SS) [batch, 1]"""
    n = v.shape[1]
    m = v.mean(1, keepdim=True)
    dm = (1 + 4 * U32) * (e.sum(1, keepdim=True) + gamma(L) * (v.abs() + e).sum(1, keepdim=True)) / n + 4 * U32 * m.abs()
    D = v - m
    SS = (D * D).sum(1, keepdim=True)
    A = 2 * (D.abs() * e).sum(1, keepdim=True) + ((e + dm) ** 2).sum(1, keepdim=True)
    return SS, A + gamma(L + 3) * (SS + A)


def cfg_rescale_axpby(x, eu, et, coef, gs, gr, depth=None):
    """x, eu, et fp32 [batch, n], coef fp32 (a, b); gs, gr as the C ABI passes them -> (ref, e, c * k) float64 [batch, n]. depth: the
    longest chain of additions in a sum (the kernel's tree by default)"""
    a, b = coef.double().tolist()
    gs, gr = fp32(gs), fp32(gr)
    L = chain(x.shape[1]) if depth is None else depth
    u, t = eu.double(), et.double()
    d = t - u
    c = u + gs * d
    e_c = U32 * (3 * abs(gs) * d.abs() + u.abs())
    SSt, Et = _ss(t, torch.zeros_like(t), L)
    SSc, Ec = _ss(c, e_c, L)
    r = (SSt / SSc).sqrt()                      # (the two 1 / (n - 1) cancel exactly)
    rho_t, rho_c = Et / SSt, Ec / SSc
    up = torch.where(rho_c < 1, ((1 + rho_t) / (1 - rho_c).clamp_min(1e-300)).sqrt(), torch.full_like(rho_c, float("inf")))
    dr = up * (1 + 1.01 * K_R * U32) - 1
    k = gr * r + (1 - gr)
    e_k = abs(gr) * r * dr + 1.01 * 2 * U32 * (abs(gr) * r * (1 + dr) + abs(1 - gr)) if gr != 0.0 else torch.zeros_like(r)
    P = b * c * k
    big = (c.abs() + e_c) * (k.abs() + e_k)
    e_P = abs(b) * (big - c.abs() * k.abs()) + 1.01 * 2 * U32 * abs(b) * big
    ax = a * x.double()
    return ax + P, e_P + 2 * U32 * (ax.abs() + P.abs() + e_P), c * k


def accumulated(xs, outs, coef64, gs, gr, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every step of a loop whose model outputs were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before step i; outs[i]: its fp32 model output [2 B, ...] ([uncond, text]);
    coef64: the scheduler's (a, b) per step as Python floats -> list of float64 bounds shaped like the latents"""
    E = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    res = []
    for x, o, (a, b) in zip(xs, outs, coef64):
        B = x.shape[0]
        c32 = torch.tensor([a, b], dtype=torch.float32)
        ref, e, ck = cfg_rescale_axpby(x.flatten(1), o[:B].flatten(1), o[B:].flatten(1), c32, gs, gr)
        a32, b32 = c32.double().tolist()
        E = abs(a) * E + 2 * U32 * ref.abs() + e + abs(a32 - a) * x.flatten(1).double().abs() + abs(b32 - b) * ck.abs()
        res.append(E.reshape(x.shape))
    return res
