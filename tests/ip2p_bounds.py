"""Float64 reference and elementwise bound for mi355x_sd_guidance3 (csrc/ip2p.hip), the sibling of tests/guidance_bounds.py, whose
statistics term (_ss: the float32 error of the two-pass variance over n elements through the kernel's tree), chain() and K_R are
imported, not restated: the kernel takes its statistics exactly as cfg_rescale_factor does. Derived from the arithmetic, not measured.
Plain Python + torch. u = U32 = 2^-24; the 1.01 factors absorb the second-order products of the u terms.

The combine, per element, in the kernel's order (t, i, u fp32; gs, gi the fp32 arguments):
    d1 = fl(i - u)   a = fl(gi d1 + u)   d2 = fl(t - i)   c = fl(gs d2 + a)            two differences, two fmas: four roundings
  d1's rounding is scaled by |gi (i - u)|, a's by |gi (i - u) + u| <= |gi (i - u)| + |u|, d2's by |gs (t - i)| and c's by
  |c| <= |gs (t - i)| + |gi (i - u)| + |u|:
    e_c = 1.01 u (2 |gs (t - i)| + 3 |gi (i - u)| + 2 |u|).
  The stored value is the last fma itself: bound_pieces.check(..., f32_rel=0). Where the three terms cancel, |c| is far below the
  magnitudes the bound is made of -- that is the point of the cancelling inputs: a regrouped or doubly rounded form
  (gs t + (gi - gs) i + (1 - gi) u, or the reference's left-to-right sum with unfused products) stays within a few e_c, but a wrong
  operand order does not.
  Inputs that carry errors e_t, e_i, e_u of their own (the x0 form) add the exact linear map's |gs| e_t + |gi - gs| e_i + |1 - gi| e_u,
  and the magnitudes above grow by the errors of their operands.

The rescale, eps form:  k as in guidance_bounds (r from the two sums of squares, dr, e_k);  out = fl(c k):
    e = (|c| + e_c)(|k| + e_k) - |c| |k| + 1.01 u (|c| + e_c)(|k| + e_k).
The x0 form, sigma = s (the fp32 value in device memory, exact):
    p_b = fl(x - s e_b)  one fma: e_p = u |x - s e_b|;   cp, e_cp as above with those input errors;   k from p_t (e_p) and cp (e_cp)
    v = fl(cp k): e_v as e above;   w = fl(v - x): e_w = e_v + u (|cp k - x| + e_v);   out = w / (-s), a division of at most 2 u:
    e = e_w / |s| + 1.01 * 2 u (|cp k - x| + e_w) / |s|."""
import torch

from tests.bound_pieces import U32, fp32
from tests.guidance_bounds import K_R, RESIDENT, _ss, chain

__all__ = ["RESIDENT", "combine", "guidance3", "cancelling_inputs"]


def combine(t, i, u, gs, gi, e_t=0.0, e_i=0.0, e_u=0.0):
    """t, i, u float64 exact values (with the error bounds of their computed versions) -> (c, e_c) float64"""
    d1, d2 = i - u, t - i
    c = u + gi * d1 + gs * d2
    carried = abs(gs) * e_t + abs(gi - gs) * e_i + abs(1 - gi) * e_u
    own = 1.01 * U32 * (2 * abs(gs) * (d2.abs() + e_t + e_i) + 3 * abs(gi) * (d1.abs() + e_i + e_u) + 2 * (u.abs() + e_u))
    return c, carried + own


def _factor(t, e_t, c, e_c, gr):
    """k = gr std(t) / std(c) + 1 - gr per sample and its error bound, [batch, 1] (tests/guidance_bounds.py cfg_rescale_axpby)"""
    L = chain(t.shape[1])
    SSt, Et = _ss(t, e_t if torch.is_tensor(e_t) else torch.zeros_like(t), L)
    SSc, Ec = _ss(c, e_c, L)
    r = (SSt / SSc).sqrt()
    rho_t, rho_c = Et / SSt, Ec / SSc
    up = torch.where(rho_c < 1, ((1 + rho_t) / (1 - rho_c).clamp_min(1e-300)).sqrt(), torch.full_like(rho_c, float("inf")))
    dr = up * (1 + 1.01 * K_R * U32) - 1
    k = gr * r + (1 - gr)
    return k, abs(gr) * r * dr + 1.01 * 2 * U32 * (abs(gr) * r * (1 + dr) + abs(1 - gr))


def _product(c, e_c, k, e_k):
    big = (c.abs() + e_c) * (k.abs() + e_k)
    return c * k, big - c.abs() * k.abs() + 1.01 * U32 * big


def guidance3(eps, gs, gi, gr=0.0, x=None, sigma=None):
    """eps fp32 [3, batch, n] (text, image, uncond), x fp32 [batch, n] or None, sigma the fp32 value or None; gs, gi, gr as the C ABI
    passes them -> (ref, e) float64 [batch, n]"""
    gs, gi, gr = fp32(gs), fp32(gi), fp32(gr)
    t, i, u = eps.double()
    if gr <= 0.0:
        return combine(t, i, u, gs, gi)
    if x is None:
        c, e_c = combine(t, i, u, gs, gi)
        k, e_k = _factor(t, 0.0, c, e_c, gr)
        return _product(c, e_c, k, e_k)
    s, xd = fp32(sigma), x.double()
    pt, pi, pu = xd - s * t, xd - s * i, xd - s * u
    e_pt, e_pi, e_pu = U32 * pt.abs(), U32 * pi.abs(), U32 * pu.abs()
    cp, e_cp = combine(pt, pi, pu, gs, gi, e_pt, e_pi, e_pu)
    k, e_k = _factor(pt, e_pt, cp, e_cp, gr)
    v, e_v = _product(cp, e_cp, k, e_k)
    w = v - xd
    e_w = e_v + U32 * (w.abs() + e_v)
    return w / (-s), e_w / abs(s) + 1.01 * 2 * U32 * (w.abs() + e_w) / abs(s)


def cancelling_inputs(batch, n, gs, gi, seed, offset=0.0):
    """eps fp32 [3, batch, n]: u ~ N(offset, 1), i = u + 0.3 N, t = i + 0.3 N; in every tenth element t is moved so that the three
    terms of the combine cancel to about 1e-3 of their size"""
    g = torch.Generator().manual_seed(seed)
    u = offset + torch.randn(batch, n, generator=g)
    i = u + 0.3 * torch.randn(batch, n, generator=g)
    t = i + 0.3 * torch.randn(batch, n, generator=g)
    partial = u.double() + fp32(gi) * (i.double() - u.double())
    cancel = (i.double() - partial * (1 - 1e-3) / fp32(gs)).float()
    tenth = (torch.arange(batch * n).reshape(batch, n) % 10) == 3
    return torch.stack([torch.where(tenth, cancel, t), i, u])
