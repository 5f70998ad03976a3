"""Elementwise float64 error bounds for the normalisation kernels (csrc/norm.hip, csrc/fused_ops.hip): GroupNorm (+SiLU, split and
one-launch forms), LayerNorm, row statistics, RMSNorm, adaLN, the fused adaLN + scale + residual op and the two e4m3 quantisers.
Each output element is held to a bound derived from the kernels' arithmetic, against a float64 reference computed from the exact
16-bit or fp32 operands the kernel reads. Plain Python + torch; runs on whatever device the tensors live on. The sibling of
tests/gemm_bounds.py and tests/attn_bounds.py, with their conventions: u32 = 2^-24, gamma(n), u_out = 2^-7 (bf16), 2^-10 (fp16).

Statistics (the contract). A normalised set S of n values x (a row, or a (batch, group) of HW * C / groups values) has mean mu,
variance var = sum (x - mu)^2 / n and rstd = 1 / sqrt(var + eps). A kernel may accumulate its sums in any fixed fp32 order whose
longest chain is L additions (the launcher's geometry: gn_geom's <= 16 pixels per thread + ppp LDS adds + cpg channel adds for the
split GroupNorm, 2 * GNF_MAXD + 6 for the one-launch GroupNorm, NCH * 8 + 6 butterfly levels for the row kernels), but it must sum
values SHIFTED by an element K of S: then sum (x - K)^2 / n = var + (mu - K)^2 <= V := var + max (x - mu)^2, whatever K it picks.
With g = gamma(L + 1) (the +1: the rounding of x - K) the shifted sums carry errors g * n * sqrt(V) and g * n * V, and the two-moment
formula m = s / n, var = q / n - m^2 (fp32 with invC = fl(1 / C), or double) gives

    |mean' - mu|  <= E_mu  = (g + 4 u32) sqrt(V) + 1.01 u32 |mu|           (the last term: mean' is an fp32 number)
    |var' - var|  <= E_var = 1.01 (3 g + 12 u32) V

Neither depends on sum x^2: a kernel that sums unshifted x and x^2 in fp32 has errors of g * n * mu^2 and fails this bound at
large |mu| / sigma (tests/test_norm_bounds.py: today's GroupNorm arithmetic at |mu| / sigma = 1000 lands ~1e5 x outside it). The
only |mu| dependence left is the fp32 representation of the mean and of the GroupNorm shift beta - mean * scale: terms
u32 |mu| rstd |gamma| (nearly translation-invariant). var' is clamped at 0, eps added (one rounding) and rsqrtf / the double
1 / sqrt cast to fp32 add RSQ relative. The relative error of rstd is then, with v = var + eps,

    delta_r = (sqrt(v / max(v - E_var - u32 v, eps (1 - u32))) - 1) (1 + RSQ) + RSQ

RMSNorm has no mean: its one sum is sum x^2 (chain L), E_var = (g + 3 u32) sum x^2 / n, and y = fl(fl(x r) w).

Outputs (z = (x - mu) rstd the exact normalised value, rho = (1 + delta_r)(1 + 2.01 u32) - 1):
  * row kernels: z' = fl(fl(x - mean') rstd'), |z' - z| <= e_z = rstd (|x - mu| rho + E_mu (1 + rho)).
    LayerNorm y = fma(z', gamma, beta): |gamma| e_z + u32 |y'|. adaLN y = fma(z', fl(1 + scale), shift): |1 + scale| (e_z +
    u32 (|z| + e_z)) + u32 |y'|. The fused op: y = fl(z' w) (u32 |z w|), fl(y + b) (u32 |y'|), then the adaLN fma; its LayerNorm
    reads the 16-bit residual the kernel WROTE (resi = fl16(fl32(fma(mha, gate, x))), held to u32 |ref| before the store).
  * GroupNorm: a = fl(gamma rstd'), b = fl(beta - fl(mean' a)), y = fma(x, a, b): x a cancels mean' a exactly inside the fma, so
    |y' - y| <= |gamma| rstd (|x - mu| rho' + E_mu (1 + rho')) + u32 |mean'| |a| + u32 |b| + u32 |y'|, rho' with u32 for 2.01 u32.
  * SiLU: silu_f = o * v_rcp(1 + __expf(-o)); |silu'| <= 1.1 carries the input error, and the exponent (u32 |o| from o * log2 e,
    EXP_REL of v_exp_f32), 1 + E, v_rcp (RCP) and the product add |silu(o)| (u32 |o| + EXP_REL + RCP + 2 u32).
  * 16-bit store: check() with u_out, as gemm_bounds: |out - ref| <= u_out |ref| + (1 + u_out) e + 2^-24.
  * e4m3 (adaln_f8): value = qs * q with qs = fl(max(amax, 1e-12) fl(1/448)), q = e4m3(fl(v fl(1 / qs))), v the fp32 adaLN value.
    |qs q - y| <= e_pre (the adaLN bound before any store) + qs (2^-4 |v / qs| + 2^-10) (half an e4m3 spacing: 3 mantissa bits;
    2^-9 spacing in the subnormal range) + 3.01 u32 |v| (the reciprocal and the product). qs itself: |qs - amax_ref / 448| <=
    (max e_pre + 2.01 u32 amax_ref) / 448. yl2 = sqrtf(fl sum v^2): |yl2 - ||y|| | <= ||e_pre|| + (gamma(L) / 2 + 2 u32) ||y||.
  * quantize_rows is held EXACTLY: quantize_rows_exact() emulates its fp32 arithmetic (qs = fl(max(amax, 1e-12) fl(1/448)),
    inv = fl(1 / qs) -- the kernel's division is the correctly rounded IEEE one, v_div_scale / v_div_fmas / v_div_fixup --, the byte =
    RNE e4m3 of fl(x inv)) and the scale and every byte must equal it.

check() returns the worst err / bound over the WHOLE output (non-finite output -> inf) and the rel-L2.
"""
import math

import numpy as np
import torch

from tests import bound_pieces as BP
from tests.bound_pieces import U32, fp32  # noqa: F401  (fp32: for the importers of this module)

U_OUT = {**BP.U_OUT, torch.float32: 0.0}
RSQ = 2 * U32        # v_rsq_f32 (1 ulp), or the double 1 / sqrt cast to fp32
RCP = 2 * U32        # v_rcp_f32 (1 ulp)
EXP_REL = 2.0 ** -21  # v_exp_f32
SILU_SLOPE = 1.1     # max |d silu / dx| = 1.0998
GN_ITERS_STATS, GNF_MAXD = 16, 24


def gamma(n: int) -> float:
    """fp32 accumulation error factor of an n-deep chain of additions"""
    return n * U32 / (1 - n * U32)


# ---- the launchers' geometry: longest fp32 chain L and NCH ------------------------------------------------------------------------
def gn_geom(HW: int, C: int, iters: int = GN_ITERS_STATS):
    """(cv, ppp, threads, block, ppb, nblk) of norm.hip gn_geom"""
    cv = C // 8
    ppp = 256 // cv if cv <= 256 else 1
    threads = ppp * cv
    ppb = ppp * iters
    return cv, ppp, threads, (threads + 63) // 64 * 64, ppb, (HW + ppb - 1) // ppb


def chain_gn_split(HW: int, C: int, groups: int) -> int:
    _, ppp, _, _, _, _ = gn_geom(HW, C)
    return GN_ITERS_STATS + ppp + C // groups + 1   # (+1: the double sums across blocks)


def chain_gn_fused() -> int:
    return 2 * GNF_MAXD + 6 + 1


NCH_RULES = {   # entry: ((cv limit, NCH), ...) of the launchers' dispatch; the last NCH takes the rest
    "layernorm": ((128, 2), (192, 3), (None, 5)),
    "row_stats": ((64, 1), (128, 2), (192, 3), (None, 5)),
    "rmsnorm": ((128, 2), (256, 4), (None, 8)),
    "adaln": ((128, 2), (192, 3), (None, 5)),
    "adaln_f8": ((128, 2), (192, 3), (None, 5)),
    "fused_adaln": ((128, 2), (256, 4), (None, 8)),
}


def nch(entry: str, C: int) -> int:
    cv = C // 8
    for lim, n in NCH_RULES[entry]:
        if lim is None or cv <= lim:
            return n


def chain_rows(entry: str, C: int) -> int:
    return nch(entry, C) * 8 + 6


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def stats(xs, L, eps):
    """xs float64 [..., n]: (mu, var, rstd, E_mu, delta_r) of the contract above, each [..., 1]"""
    mu = xs.mean(-1, keepdim=True)
    dev = (xs - mu) ** 2
    var = dev.mean(-1, keepdim=True)
    V = var + dev.amax(-1, keepdim=True)
    g = gamma(L + 1)
    e_mu = (g + 4 * U32) * V.sqrt() + 1.01 * U32 * mu.abs()
    e_var = 1.01 * (3 * g + 12 * U32) * V
    return mu, var, 1.0 / (var + eps).sqrt(), e_mu, rstd_rel(var, e_var, eps)


def rstd_rel(var, e_var, eps):
    v = var + eps
    lo = torch.maximum(v - e_var - U32 * v, torch.full_like(v, eps * (1 - U32)))
    return ((v / lo).sqrt() - 1) * (1 + RSQ) + RSQ


def _silu(ref, e):
    o = ref * torch.sigmoid(ref)
    return o, SILU_SLOPE * e + o.abs() * (U32 * (ref.abs() + e) + EXP_REL + RCP + 2 * U32)


def groupnorm(x, gamma_, beta, groups, eps, silu=False, L=None):
    """x [B, HW, C] (the exact 16-bit or fp32 values), gamma / beta fp32 [C]: (ref, e) float64 [B, HW, C] of the split
    (L = chain_gn_split) or the one-launch (L = chain_gn_fused) form"""
    B, HW, C = x.shape
    cpg = C // groups
    eps = fp32(eps)
    xs = x.double().reshape(B, HW, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, HW * cpg)
    mu, var, rstd, e_mu, dr = stats(xs, L, eps)
    rep = lambda t: t.repeat_interleave(cpg, 1).reshape(B, 1, C)   # noqa: E731  [B, groups, 1] -> [B, 1, C]
    mu, rstd, e_mu, dr = rep(mu), rep(rstd), rep(e_mu), rep(dr)
    g, b = gamma_.double().reshape(1, 1, C), beta.double().reshape(1, 1, C)
    xd = x.double()
    ref = (xd - mu) * rstd * g + b
    rho = (1 + dr) * (1 + U32) - 1
    a = g.abs() * rstd * (1 + rho)
    e = g.abs() * rstd * ((xd - mu).abs() * rho + e_mu * (1 + rho)) + U32 * (mu.abs() + e_mu) * a
    e = e + U32 * (b.abs() + (mu.abs() + e_mu) * a) * (1 + U32) + U32 * (ref.abs() + e)
    if silu:
        ref, e = _silu(ref, e)
    return ref, e


def _row_z(x, L, eps):
    """x [rows, C] exact values: (z, e_z, mu, rstd, e_mu, delta_r) of the row kernels' z' = fl(fl(x - mean') rstd')"""
    xd = x.double()
    mu, var, rstd, e_mu, dr = stats(xd, L, fp32(eps))
    rho = (1 + dr) * (1 + 2.01 * U32) - 1
    z = (xd - mu) * rstd
    e_z = rstd * ((xd - mu).abs() * rho + e_mu * (1 + rho))
    return z, e_z, mu, rstd, e_mu, dr


def layernorm(x, gamma_, beta, eps, L):
    """x [rows, C]; gamma / beta fp32 [C] or None"""
    z, e_z, *_ = _row_z(x, L, eps)
    g = gamma_.double() if gamma_ is not None else torch.ones((), dtype=torch.float64, device=x.device)
    b = beta.double() if beta is not None else torch.zeros((), dtype=torch.float64, device=x.device)
    ref = z * g + b
    e = g.abs() * e_z
    return ref, e + U32 * (ref.abs() + e)


def row_stats(x, eps, L):
    """x [rows, C] -> (ref, e) [rows, 2] = (rstd, -mean * rstd) (fp32 outputs: check with u_out = 0)"""
    z, e_z, mu, rstd, e_mu, dr = _row_z(x, L, eps)
    ref = torch.cat([rstd, -mu * rstd], 1)
    e1 = rstd * (e_mu * (1 + dr) + mu.abs() * dr)
    e1 = e1 + 2.01 * U32 * (ref[:, 1:].abs() + e1)
    return ref, torch.cat([rstd * dr, e1], 1)


def rmsnorm(x, w, eps, L):
    xd = x.double()
    ms = (xd * xd).mean(-1, keepdim=True)
    eps = fp32(eps)
    r = 1.0 / (ms + eps).sqrt()
    dr = rstd_rel(ms, (gamma(L) + 3 * U32) * ms, eps)
    ref = xd * r * w.double()
    rho = (1 + dr) * (1 + 2.01 * U32) - 1
    return ref, ref.abs() * rho


def _mod_rows(t, rows, rpb):
    """per-row modulation [rows, C] from [batches, >= C] (a strided view; the gaps are never part of it)"""
    idx = torch.arange(rows, device=t.device) // rpb
    return t.double()[idx]


def adaln_pre(x, scale, shift, rpb, eps, L):
    """(ref, e) before any store of y = LN(x) (1 + scale[b]) + shift[b], b = row // rpb"""
    C = x.shape[1]
    z, e_z, *_ = _row_z(x, L, eps)
    sc, sh = _mod_rows(scale[:, :C], x.shape[0], rpb), _mod_rows(shift[:, :C], x.shape[0], rpb)
    ref = z * (1 + sc) + sh
    e = (1 + sc).abs() * (e_z + U32 * (z.abs() + e_z))
    return ref, e + U32 * (ref.abs() + e)


def adaln(x, scale, shift, rpb, eps, L):
    return adaln_pre(x, scale, shift, rpb, eps, L)


def fused_resi(x, mha, gate, rpb):
    """resi = mha * gate[b] + x: (ref, e) before the 16-bit store (one fp32 fma)"""
    C = x.shape[1]
    ref = mha.double() * _mod_rows(gate[:, :C], x.shape[0], rpb) + x.double()
    return ref, U32 * ref.abs()


def fused_adaln_out(resi, scale, shift, rpb, weight, bias, eps, L):
    """adaLN_out from the 16-bit resi the kernel wrote: (ref, e) before the store"""
    C = resi.shape[1]
    z, e_z, *_ = _row_z(resi, L, eps)
    t, e = z, e_z
    if weight is not None:
        w = weight.double()
        t, e = z * w, w.abs() * e_z
        e = e + U32 * (t.abs() + e)
    if bias is not None:
        t = t + bias.double()
        e = e + U32 * (t.abs() + e)
    sc, sh = _mod_rows(scale[:, :C], resi.shape[0], rpb), _mod_rows(shift[:, :C], resi.shape[0], rpb)
    ref = t * (1 + sc) + sh
    e = (1 + sc).abs() * (e + U32 * (t.abs() + e))
    return ref, e + U32 * (ref.abs() + e)


# ---- checks -------------------------------------------------------------------------------------------------------------------
def check(out, ref, e, u_out=None):
    """(worst |out - ref| / bound over every element, rel-L2); u_out defaults to the output's own rounding out of this module's
    U_OUT: an fp32 output takes the 16-bit form at u = 0 (e + 2^-24). rel-L2's denominator is clamped at 1e-300."""
    return BP.check(out, ref, e, u_out=U_OUT[out.dtype] if u_out is None else u_out, rel_floor=1e-300)


def e4m3_value(q):
    """uint8 e4m3 (OCP, fn) bytes -> float64 values"""
    return q.view(torch.float8_e4m3fn).double()


def check_f8(q, qs, l2, ref, e):
    """adaln_f8: (worst err / bound of qs * q, of qs, of yl2 (or 0 when l2 is None), number of NaN bytes)"""
    v = e4m3_value(q)
    s = qs.double()[:, None]
    ya = ref.abs() + e
    bound = e + s * (2.0 ** -4 * ya / s + 2.0 ** -10) + 3.01 * U32 * ya + U32
    r_val = ((s * v - ref).abs() / bound).max().item()
    amax = ref.abs().amax(1)
    r_qs = ((qs.double() - amax / 448).abs() / ((e.amax(1) + 2.01 * U32 * amax) / 448 + 1e-30)).max().item()
    r_l2 = 0.0
    if l2 is not None:
        n = ref.norm(dim=1)
        Lq = ref.shape[1] // 64 + 6 + 8
        r_l2 = ((l2.double() - n).abs() / (e.norm(dim=1) + (gamma(Lq) / 2 + 2 * U32) * n + 1e-30)).max().item()
    nan = int(((q & 0x7F) == 0x7F).sum().item())
    bad = lambda r: float("inf") if r != r else r   # noqa: E731
    return bad(r_val), bad(r_qs), bad(r_l2), nan


def e4m3_rne(v32: np.ndarray) -> np.ndarray:
    """RNE e4m3 (OCP fn, saturating finite inputs never exceed 448 here) bytes of fp32 values"""
    return torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def quantize_rows_exact(x):
    """the kernel's fp32 arithmetic on CPU: x [rows, C] (16-bit) -> (uint8 [rows, C], fp32 [rows])"""
    xf = x.float().cpu().numpy().astype(np.float32)
    amax = np.abs(xf).max(1)
    qs = (np.maximum(amax, np.float32(1e-12)) * (np.float32(1.0) / np.float32(448.0))).astype(np.float32)
    inv = (np.float32(1.0) / qs).astype(np.float32)
    return torch.from_numpy(e4m3_rne((xf * inv[:, None]).astype(np.float32))), torch.from_numpy(qs)
