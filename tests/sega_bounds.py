"""Float64 reference and elementwise bound for mi355x_sd_sega_guidance (csrc/sega.hip). Derived from the arithmetic, not measured.
Plain Python + torch. u = U32 = 2^-24; the 1.01 factors absorb the second-order products of the u terms.

What is exact. g = fl(fl(e - u) * s) is the reference's own two roundings, so the keys, the order statistics v[lo], v[hi] and -- the
threshold being the same bits or the element not within an ulp of it -- the mask are the reference's: g_c below is an fp32 value
both sides share, and the reference here takes the mask from ``torch.quantile`` on the fp32 |g|, as the reference pipeline does.

What rounds, per element, in the kernel's order (include/mi355x_sd.h), against the real-number value of the reference's lines
(pipeline_semantic_stable_diffusion.py:546, :654-699) on the fp32 row scalars:
    G    = fl(gs * fl(t - u))                       two roundings of a value of size |gs (t - u)|:    e_G = 1.01 * 2 u |G|
    edit = fma(w_c, g_c, edit) for c < n, then fma(ms, m, edit):  n + 1 roundings, each of a partial sum no larger than
           A_E = sum |w_c g_c| + |ms m|:                                                              e_E = 1.01 (n + 1) u A_E
    part = the same over the warm concepts, k of them:                                                e_P = 1.01 k u A_P
    m'   = fma(beta, m, fl(omb * edit)):            e_M = |omb| e_E + 1.01 u (2 |omb| (|E| + e_E) + |beta m|)
    every later sum fl(a + b) of values known to (e_a, e_b):          e = e_a + e_b + 1.01 u (|a| + |b| + e_a + e_b)
    in the order  G (+ part) (+ edit) (+ extra),  out = u + that.
The stored values are the last operations themselves: bound_pieces.check(..., f32_rel=0).
thr: one fma of the lerp on exact operands (v[hi] - v[lo] may round: one more): within 1 ulp of the float64 lerp, and the same bits
where v[lo] == v[hi] (the difference is 0)."""
import torch

from paddlemix_amd import sega_forms as SF
from tests.abi_emulator_sega import parse_row
from tests.bound_pieces import U32

K = 1.01 * U32


def _add(a, ea, b, eb):
    return a + b, ea + eb + K * (a.abs() + b.abs() + ea + eb)


def ulp32(x64):
    """the spacing of fp32 at |x| (float64 tensor in, float64 out)"""
    x = x64.abs().float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def lerp64(vlo, vhi, frac):
    a, b, w = vlo.double(), vhi.double(), float(frac)
    return a + w * (b - a) if abs(w) < 0.5 else b - (b - a) * (1.0 - w)


def reference(eps, momentum, extra, row, n, q):
    """eps fp32 [2 + n, B, C, hw], momentum / extra fp32 [B, C, hw], row int32 words, q the case's threshold ->
    dict(out, e_out, mom, e_mom: float64; vlo, vhi: fp32 [n, B, C]; thr64: float64 [n, B, C]; thr_ref: fp32 (torch.quantile);
    mask: bool [n, B, C, hw] (the reference's); near: elements of a live concept within an ulp of an inexact threshold)"""
    r = parse_row(row, n)
    u32, t32 = eps[0], eps[1]
    B, C, hw = u32.shape
    u, t, m = u32.double(), t32.double(), momentum.double()
    z = torch.zeros_like(u)
    gs = float(r["gs"])
    G = gs * (t - u)
    e_G = 2 * K * G.abs()
    E, A_E, P, A_P = z.clone(), z.clone(), z.clone(), z.clone()
    vlo, vhi = torch.zeros(n, B, C), torch.zeros(n, B, C)
    thr64, thr_ref = torch.zeros(n, B, C, dtype=torch.float64), torch.zeros(n, B, C)
    mask, near = torch.zeros(n, B, C, hw, dtype=torch.bool), 0
    warm = [c for c in range(n) if (r["warm"] >> c) & 1]
    for c, pc in enumerate(r["per"]):
        wf, wp = float(pc["w_full"]), float(pc["w_part"])
        g = z
        if (r["active"] >> c) & 1:
            g32 = (eps[2 + c] - u32) * torch.tensor(float(pc["scale"]), dtype=torch.float32)     # the reference's two roundings
            a = g32.abs()
            srt = torch.sort(a, dim=2).values                                                   # NaNs last
            lo = pc["lo"]
            hi = lo + 1 if float(pc["frac"]) != 0.0 and lo + 1 <= hw - 1 else lo
            vlo[c], vhi[c] = srt[..., lo], srt[..., hi]
            thr64[c] = lerp64(vlo[c], vhi[c], pc["frac"])
            thr64[c][torch.isnan(a).any(dim=2)] = float("nan")
            thr_ref[c] = torch.quantile(a, q, dim=2, keepdim=False)
            mask[c] = a >= thr_ref[c][..., None]
            inexact = (vlo[c] != vhi[c])[..., None]
            near += int((((a.double() - thr64[c][..., None]).abs() <= ulp32(thr64[c])[..., None]) & inexact).sum())
            g = torch.where(mask[c], g32, torch.zeros_like(g32)).double()
        E, A_E = E + wf * g, A_E + (wf * g).abs()
        if c in warm:
            P, A_P = P + wp * g, A_P + (wp * g).abs()
    ms, beta, omb = float(r["ms"]), float(r["beta"]), float(r["omb"])
    E, A_E = E + ms * m, A_E + (ms * m).abs()
    e_E, e_P = K * (n + 1) * A_E, K * max(len(warm), 1) * A_P
    mom = beta * m + omb * E
    e_mom = abs(omb) * e_E + K * (2 * abs(omb) * (E.abs() + e_E) + (beta * m).abs())
    guid, e = G, e_G
    if r["regime"] == SF.REGIME_PARTIAL:
        guid, e = _add(guid, e, P, e_P)
    if r["regime"] == SF.REGIME_ALL:
        guid, e = _add(guid, e, E, e_E)
    if extra is not None:
        guid, e = _add(guid, e, extra.double(), z)
    out, e_out = _add(u, z, guid, e)
    return dict(out=out, e_out=e_out, mom=mom, e_mom=e_mom, vlo=vlo, vhi=vhi, thr64=thr64, thr_ref=thr_ref, mask=mask, near=near)


def check_values(got, ref, e):
    """worst |got - ref| / e over the elements whose reference is finite (0 / 0 passes); elsewhere the class must agree: NaN with
    NaN, an infinity with the same infinity -> (ratio, number of elements of the wrong class)"""
    fin = torch.isfinite(ref) & torch.isfinite(e)
    err = (got.double() - ref).abs()
    bound = torch.where((e == 0) & (err == 0), torch.ones_like(e), e)
    ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    if ratio != ratio:
        ratio = float("inf")
    g, rf = got.double()[~fin], ref[~fin]
    same = (torch.isnan(g) & torch.isnan(rf)) | (g == rf)
    return ratio, int((~same).sum())


def check_thr(thr, vlo, vhi, thr64):
    """thr fp32 against the float64 lerp: within 1 ulp, equal bits where v[lo] == v[hi]; a NaN where the float64 value is one -> number
    of planes that miss"""
    bad = 0
    t, r = thr.double().flatten(), thr64.flatten()
    for k in range(t.numel()):
        if r[k] != r[k]:
            bad += int(t[k] == t[k])
        elif not torch.isfinite(r[k]):
            bad += int(t[k] != r[k])
        elif vlo.flatten()[k] == vhi.flatten()[k]:
            bad += int(t[k] != vlo.double().flatten()[k])
        else:
            bad += int(not (t[k] - r[k]).abs() <= ulp32(r[k:k + 1])[0])
    return bad
