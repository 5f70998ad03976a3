"""Elementwise float64 error bound for the attention kernels (csrc/attention.hip, every form launch_dp launches): every output element
is held to a bound derived from the kernels' arithmetic, against a float64 reference computed from the exact 16-bit operands. Plain
Python + torch; runs on whatever device the tensors live on. The sibling of tests/gemm_bounds.py.

Reference. For each (b, h, query i), in natural-log units (the log2 form, q carrying scale * log2(e), is scale = ln 2):

    x_j = scale * q.k_j + bias_ij,   m = max_j x_j,   w_j = exp(x_j - m),   ref = sum_j w_j v_j / sum_j w_j

Kernel arithmetic, and what each step costs (u32 = 2^-24):
  * Scores. q.k_j is a chain of fp32 MFMA accumulations over D (16- or 32-deep steps): |err| <= gamma_D S_j with
    S_j = sum_d |q_d k_jd| and gamma_D = (D / 16 + 32) u32 (as gemm_bounds.gamma). The log2 form seeds the chain with -m, which adds
    gamma_D |m| to the same chain. The masked form adds fl(bias * fl(1 / scale)) to the score (two roundings of |bias| / scale, one of
    the sum). The exponent is fma(s, c2, -fl(m c2)) with c2 = fl(scale * fl(log2 e)): roundings of |x_j|, |m| and of the result,
    whose size is |x_j - m'| log2 e for the kernel's reference m' -- the exact maximum, or in the lazy form a stale one at most 60
    log2 units (the guard LAZY_PSUM_LIMIT) below a score. v_exp_f32 adds EXP_REL relative. Together a per-key relative error of the
    weight, eps_j = scale gamma_D S_j + gamma_D |m| + C_RND u32 (|x_j| + |m| + 2 |bias_ij| + |x_j - m| + 64) + EXP_REL.
    Whatever multiplies every weight of a row alike (the reference itself, stale or not) cancels between numerator and row sum.
  * P. The weights enter the P.V MFMA rounded to the 16-bit element type: |fl(e) - e| <= u_p max(e, tiny) with u_p = 2^-8 (bf16),
    2^-11 (fp16; tiny = 2^-14, its subnormal range; 0 for bf16). The row sum l is accumulated from the UNROUNDED fp32 e, so this
    rounding does not cancel: it costs u_p sum_j (w_j + tiny) |v_jd| / sum_j w_j (the kernel's weights are w_j times a factor >= 1,
    its reference never exceeds the true maximum, so tiny relative to them is at most tiny relative to w).
  * Accumulation. P.V sums in fp32 MFMA chains over Skv (gamma_Skv on sum_j P_j |v_jd|); l sums in fp32 lane partials (at most 64
    + ntiles + 2 roundings); each online rescale multiplies o and l by the same alpha: one rounding each per event, at most one per
    64-key tile. out = o * fl(1 / l): a v_rcp_f32 and a product, 3 u32 |ref|.
  * accum (IP-Adapter): out = old + accum * attn with `old` read exactly: |accum| e_attn + 2 u32 (|old| + |accum ref|).
  * Store: one rounding to the element type, u_out = 2 u as in gemm_bounds (2^-7 bf16, 2^-10 fp16), applied by check():
        |out - ref| <= u_out |ref| + (1 + u_out) e + 2^-24

exact_p. Where every valid key of a row has the same score (identical key rows: S1 of tests/attn_cases.py) every P is exactly 1 and
the u_p term drops out. Identical K rows give bit-identical scores: an MFMA output element is the same fixed-order fp32 chain of the
same products whichever row / column it sits in, and in the log2 form every chain of a tile starts from the same -m. The maximum is
then that very score, and the exponent fma(s, c2, -fl(s c2)) is the rounding error of s c2, a few fp32 ulps of it (a few ulps of
m - s in the log2 form, whose chain reproduces s only to its own roundings) -- exp2 of that is 1 within ~2^-20, which the 16-bit
conversion returns as exactly 1. Keys under a -10000 keep-mask exponentiate to exactly 0 and keep the argument intact.

A row whose keys are ALL masked with -inf has no softmax; the kernels write 0 there (inv_l = 0, include/mi355x_sd.h) and reference()
returns 0 with e = 0.

This bound is worst-case: on flat softmaxes (random inputs) it is about sqrt(S_eff) looser than the kernels' actual error. Its
sharpness comes from the inputs (tests/attn_cases.py: uniform keys with exact_p, one-hot selectors), where it is within a small
factor of the kernels' real error. check() returns the worst err / bound over the WHOLE output and its rel-L2.
"""
import math

import torch

from tests import bound_pieces as BP
from tests.bound_pieces import U32, U_OUT, fp32  # noqa: F401  (U_OUT, fp32: for the importers of this module)

U_P = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
P_TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -14}
C_RND = 8
EXP_REL = 2.0 ** -20
LN2 = math.log(2.0)


def gamma(n: int) -> float:
    """fp32 accumulation error factor of an n-deep sum in chains of 16-deep MFMA steps"""
    return (n / 16 + 32) * U32


def reference(q, k, v, *, scale=None, bias=None, log2=False, accum=None, old=None, exact_p=False):
    """float64 reference and elementwise error e (before the output rounding) of mi355x_sd_sdpa / _ex (log2) / _accum.
    q [B, Sq, H, D], k / v [B, Skv, H, D] (16-bit, the logical operands exactly as the kernel reads them), bias fp32 broadcastable to
    [B, H, Sq, Skv], old [B, Sq, H, D] (what `out` held before an accumulating call). Returns (ref, e), both [B, Sq, H, D] float64."""
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    dt = q.dtype
    if log2:
        sc = LN2
    else:
        sc = fp32(scale if scale is not None else 1.0 / math.sqrt(D))
    ntiles = (Skv + 63) // 64
    g_d, g_s = gamma(D), gamma(Skv)
    g_l = (64 + 2 * ntiles + 2) * U32
    u_p = 0.0 if exact_p else U_P[dt]
    tiny = P_TINY[dt]
    refs, errs = [], []
    for b in range(B):   # (one batch item at a time: [H, Sq, Skv] float64 intermediates)
        Q = q[b].double().transpose(0, 1)
        K = k[b].double().transpose(0, 1)
        V = v[b].double().transpose(0, 1)
        x = sc * (Q @ K.transpose(1, 2))
        S = Q.abs() @ K.abs().transpose(1, 2)
        del Q, K
        if bias is not None:
            bb = bias[b if bias.shape[0] > 1 else 0].double().expand(H, Sq, Skv)
            x = x + bb
            babs = bb.abs().nan_to_num(posinf=0.0)
        else:
            babs = torch.zeros((), dtype=torch.float64, device=x.device)
        m = x.amax(-1, keepdim=True)
        dead = m == -math.inf   # rows masked entirely with -inf: 0 by convention
        mm = torch.where(dead, torch.zeros_like(m), m)
        w = torch.exp(x - mm)
        fin = w > 0
        eps = (sc * g_d * S + g_d * mm.abs() + C_RND * U32 * (x.abs() + mm.abs() + 2 * babs + (x - mm).abs() + 64)
               + EXP_REL)
        eps = torch.where(fin, eps, torch.zeros_like(eps))
        del S, x, babs
        W = w.sum(-1, keepdim=True)
        Va = V.abs()
        ref = (w @ V) / W.clamp_min(1e-300)
        A = w @ Va
        eN = (w * eps) @ Va + u_p * ((w + tiny * fin) @ Va) + (g_s + ntiles * U32) * (1 + U_P[dt]) * A
        eL = (w * eps).sum(-1, keepdim=True) + g_l * W
        e = (eN + ref.abs() * eL) / (W - eL).clamp_min(1e-300) + 3 * U32 * ref.abs()
        ref = torch.where(dead, torch.zeros_like(ref), ref)
        e = torch.where(dead, torch.zeros_like(e), e)
        refs.append(ref.transpose(0, 1))
        errs.append(e.transpose(0, 1))
        del w, eps, A, eN, eL, V, Va
    ref = torch.stack(refs)
    e = torch.stack(errs)
    if accum is not None:
        a = fp32(accum)
        o = old.double()
        e = abs(a) * e + 2 * U32 * (o.abs() + abs(a) * ref.abs())
        ref = o + a * ref
    return ref, e


def check(out, ref, e):
    """(worst |out - ref| / bound over every element, rel-L2) of a 16-bit output against reference() (non-finite -> inf); rel-L2's
    denominator is clamped at 1e-300 (a fully masked output has a zero reference)"""
    return BP.check(out, ref, e, rel_floor=1e-300)


def bound_check(out, q, k, v, **kw):
    """reference() + check() in one call: (worst err / bound, rel-L2)"""
    ref, e = reference(q, k, v, **kw)
    return check(out, ref, e)
