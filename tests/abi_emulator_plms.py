"""mi355x_sd_plms_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=PlmsEmulator())``.

emulate() restates the device kernels (csrc/step_tail.hip PlmsStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the statistics of the rescale go through tree_sum of
tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_plms_bounds.py:
  "swap_h12"         the planes of h1 and h2 exchanged
  "from_x"           the averaging row (from_park) starts from x instead of the parked sample
  "append_avg"       the averaging row stores e in the ring, as every other row does
  "convert_x"        the v-prediction conversion taken with x instead of S (differs on the averaging row)
  "drop_w3"          the fourth term left out
  "store_converted"  the ring takes the converted output instead of e
  "mul_nan"          every term and both of x and P are formed, with a zero weight where the row does not use them"""
from __future__ import annotations

import torch

from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32, GuidanceEmulator, tree_sum
from tests.plms_bounds import flags


def _guided(eu, et, gs, gr):
    if et is None:
        return eu
    n = eu.shape[1]
    gs, gr = torch.tensor(gs, dtype=F32), torch.tensor(gr, dtype=F32)
    one = torch.tensor(1.0, dtype=F32)
    e = (eu.double() + gs.double() * (et - eu).double()).to(F32)   # fma(gs, fl(t - u), u): one rounding after the exact product
    if gr > 0:
        inv_n, inv_nm1 = one / torch.tensor(float(n), dtype=F32), one / torch.tensor(float(n - 1), dtype=F32)
        ss = []
        for v in (et, e):
            d = v - (tree_sum(v) * inv_n)[:, None]
            ss.append(tree_sum(d * d))
        r = torch.sqrt(ss[0] * inv_nm1) / torch.sqrt(ss[1] * inv_nm1)
        e = e * (gr * r + (one - gr))[:, None]
    return e


def emulate(x, eu, et, P, H, coef, gs, gr, fault=None):
    """x, eu, et (or None), P fp32 [batch, n]; H fp32 [3, batch, n]; coef fp32, 12 values -> (out, P, H) fp32: the state as the
    launch leaves it (new tensors)"""
    a, b, p, q, w0, w1, w2, w3 = coef.to(F32)[:8]
    slot, park, from_park = flags(coef)
    e = _guided(eu, et, gs, gr)
    planes = [(slot - k) % 3 for k in (1, 2, 3)]
    if fault == "swap_h12":
        planes[0], planes[1] = planes[1], planes[0]
    m = w0 * e
    for k, (w, pl) in enumerate(zip((w1, w2, w3), planes)):
        if (w != 0 or fault == "mul_nan") and not (k == 2 and fault == "drop_w3"):
            m = m + w * H[pl]
    S = x if (not from_park or fault == "from_x") else P
    if p != 0 or fault == "mul_nan":
        m = p * (x if fault == "convert_x" else S) + q * m
    out = a * S + b * m
    if fault == "mul_nan":
        out = out + 0.0 * (P if S is x else x)
    H, P = H.clone(), P.clone()
    if not from_park or fault == "append_avg":
        H[slot] = m if fault == "store_converted" else e
    if park:
        P = x.clone()
    return out, P, H


class PlmsEmulator(GuidanceEmulator):
    def mi355x_sd_plms_update(self, x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream):
        self.calls.append("plms_update")
        assert x and eu and park and hist and out and coef and batch > 0 and per_sample >= (2 if et and gr > 0 else 1)
        n = batch * per_sample
        apart = lambda p, np_, q, nq: p + 4 * np_ <= q or q + 4 * nq <= p  # noqa: E731
        written = ((out, n), (park, n), (hist, 3 * n))
        assert out == x or apart(out, n, x, n)
        assert all(apart(w, nw, p, n) for w, nw in written for p in (eu, et) if p) and all(apart(w, nw, coef, 12) for w, nw in written)
        assert apart(park, n, x, n) and apart(hist, 3 * n, x, n) and apart(out, n, park, n) and apart(out, n, hist, 3 * n)
        assert apart(park, n, hist, 3 * n)
        k = _flat(coef, 12, F32)
        v = [_flat(p, n, F32).reshape(batch, per_sample) if p else None for p in (x, eu, et, park)]
        H = _flat(hist, 3 * n, F32).reshape(3, batch, per_sample)
        o, P, Hn = emulate(*v, H, k, gs, gr if et else 0.0)
        slot, parks, from_park = flags(k)
        if not from_park:   # only what the kernel writes is written: the other planes keep whatever they hold
            H[slot].copy_(Hn[slot])
        if parks:
            _flat(park, n, F32).copy_(P.reshape(-1))
        _flat(out, n, F32).copy_(o.reshape(-1))
        return 0
