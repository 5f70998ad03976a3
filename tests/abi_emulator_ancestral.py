"""mi355x_sd_ancestral_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=AncestralEmulator())``.

emulate() restates the device kernels (csrc/misc.hip ancestral_kernel / ancestral_rescale_kernel) in torch fp32, one rounding per
operation and in the kernel's own order; the statistics of the rescale go through tree_sum of tests/abi_emulator_guidance.py. It is
NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault`` restates a FAULT for
tests/test_ancestral_bounds.py: "mul_nan" (c * z computed at c = 0 instead of skipped), "bf16_noise" (z rounded to bfloat16 before
use), "one_pass" (the fp32 sum v^2 - n mean^2 variance)."""
from __future__ import annotations

import torch

from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32, GuidanceEmulator, tree_sum


def emulate(x, eu, et, z, coef, gs, gr, fault=None):
    """x, eu, et (or None), z (or None at c = 0) fp32 [batch, n]; coef fp32 (a, b, c) -> out fp32 [batch, n]"""
    n = x.shape[1]
    a, b, c = coef.to(F32)
    e = eu
    if et is not None:
        gs, gr = torch.tensor(gs, dtype=F32), torch.tensor(gr, dtype=F32)
        one = torch.tensor(1.0, dtype=F32)
        e = (eu.double() + gs.double() * (et - eu).double()).to(F32)   # fma(gs, fl(t - u), u): one rounding after the exact product
        if gr > 0:
            inv_n, inv_nm1 = one / torch.tensor(float(n), dtype=F32), one / torch.tensor(float(n - 1), dtype=F32)
            ss = []
            for v in (et, e):
                s = tree_sum(v)
                if fault == "one_pass":
                    ss.append(tree_sum(v * v) - (s * inv_n) * s)
                else:
                    d = v - (s * inv_n)[:, None]
                    ss.append(tree_sum(d * d))
            r = torch.sqrt(ss[0] * inv_nm1) / torch.sqrt(ss[1] * inv_nm1)
            e = e * (gr * r + (one - gr))[:, None]
    out = a * x + b * e
    if c != 0 or fault == "mul_nan":
        out = out + c * (z.to(torch.bfloat16).to(F32) if fault == "bf16_noise" else z)
    return out


class AncestralEmulator(GuidanceEmulator):
    def mi355x_sd_ancestral_update(self, x, eu, et, noise, out, coef, gs, gr, batch, per_sample, stream):
        self.calls.append("ancestral_update")
        assert x and eu and out and coef and batch > 0 and per_sample >= (2 if et and gr > 0 else 1)
        n = batch * per_sample
        apart = lambda p, q, nq: p + 4 * n <= q or q + 4 * nq <= p  # noqa: E731
        assert out == x or apart(out, x, n)
        assert all(apart(out, p, n) for p in (eu, et, noise) if p) and apart(out, coef, 3)
        k = _flat(coef, 3, F32)
        assert noise or k[2] == 0, "a null noise plane on a row with c != 0"
        v = [_flat(p, n, F32).reshape(batch, per_sample) if p else None for p in (x, eu, et, noise)]
        _flat(out, n, F32).copy_(emulate(*v, k, gs, gr if et else 0.0).reshape(-1))
        return 0
