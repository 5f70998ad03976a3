"""mi355x_sd_dpm2_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=Dpm2Emulator())``.

emulate() restates the device kernels (csrc/step_tail.hip MidpointStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the statistics of the rescale go through tree_sum of
tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_dpm2_bounds.py: "from_x" (stage 2 starts from x instead of the parked sample), "mul_nan" (the terms
over state a row must not read are formed with a zero weight instead of skipped: stage 1 adds 0 * S, every row at c == 0 or in stage 1
adds c * z), "bf16_noise" (the noise rounded to bfloat16 before use)."""
from __future__ import annotations

import torch

from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32, GuidanceEmulator, tree_sum


def emulate(x, eu, et, z, S, coef, gs, gr, fault=None):
    """x, eu, et (or None), z (or None where the row reads none), S fp32 [batch, n]; coef fp32 (p, q, h, c, second) -> (out, S) fp32
    [batch, n]: the plane as the launch leaves it (stage 1: a new one; stage 2: the very tensor passed in)"""
    n = x.shape[1]
    p, q, h, c, second = coef.to(F32)
    e = eu
    if et is not None:
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
    d = p * x + q * e if p != 0 else q * e
    if second == 0:
        out = x + h * d
        if fault == "mul_nan":
            out = out + 0.0 * S + c * z
        return out, x.clone()
    out = (x if fault == "from_x" else S) + h * d
    if c != 0 or fault == "mul_nan":
        out = out + c * (z.to(torch.bfloat16).to(F32) if fault == "bf16_noise" else z)
    return out, S


class Dpm2Emulator(GuidanceEmulator):
    def mi355x_sd_dpm2_update(self, x, eu, et, noise, sample, out, coef, gs, gr, batch, per_sample, stream):
        self.calls.append("dpm2_update")
        assert x and eu and sample and out and coef and batch > 0 and per_sample >= (2 if et and gr > 0 else 1)
        n = batch * per_sample
        apart = lambda p, q, nq: p + 4 * n <= q or q + 4 * nq <= p  # noqa: E731
        assert out == x or apart(out, x, n)
        assert all(apart(w, p, n) for w in (out, sample) for p in (eu, et, noise) if p) and all(apart(w, coef, 5) for w in (out, sample))
        assert apart(sample, x, n) and apart(out, sample, n)
        k = _flat(coef, 5, F32)
        assert noise or k[4] == 0 or k[3] == 0        # a null plane only where the row reads none
        v = [_flat(p, n, F32).reshape(batch, per_sample) if p else None for p in (x, eu, et, noise, sample)]
        o, S = emulate(*v, k, gs, gr if et else 0.0)
        if k[4] == 0:
            _flat(sample, n, F32).copy_(S.reshape(-1))
        _flat(out, n, F32).copy_(o.reshape(-1))
        return 0
