"""mi355x_sd_unipc_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=UniPCEmulator())``.

emulate() restates the device kernels (csrc/misc.hip unipc_kernel / unipc_rescale_kernel) in torch fp32, one rounding per operation
and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is NOT
scheduler.step: that is the generic loop the fused loop is compared against. ``fault`` restates a FAULT for
tests/test_unipc_bounds.py: "regroup" (the coefficient applied before the difference: C h_k - C h1, D h_k - D m_t), "mul_nan" (every
term formed whatever its coefficient, the corrector blended in as corr * x_c + (1 - corr) * x instead of skipped)."""
from __future__ import annotations

import torch

from tests.abi_emulator_guidance import F32, guided
from tests.abi_emulator_multistep import MultistepEmulator
from tests.step_forms import FORMS


def emulate(x, eu, et, last, hist, coef, gs, gr, order, fault=None):
    """x, eu, et (or None), last fp32 [batch, n]; hist fp32 [order, batch, n]; coef fp32 (12,) -> (out, last', hist') fp32"""
    p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr = coef.to(F32)
    zero = torch.zeros_like(x)
    e = guided(eu, et, gs, gr)
    every = fault == "mul_nan"
    h = [hist[j] if j < order else None for j in range(3)]

    def scaled_diff(c, a, b):
        return c * a - c * b if fault == "regroup" else c * (a - b)

    mt = p * x + q * e
    xc = x
    if corr != 0 or every:
        a = zero
        if Ac != 0 or every:
            a = Ac * last
        if Bc != 0 or every:
            a = a + Bc * h[0]
        if (C2 != 0 or every) and order >= 2:
            a = a + scaled_diff(C2, h[1], h[0])
        if (C3 != 0 or every) and order >= 3:
            a = a + scaled_diff(C3, h[2], h[0])
        if Ct != 0 or every:
            a = a + scaled_diff(Ct, mt, h[0])
        xc = corr * a + (1 - corr) * x if every else a
    out = Ap * xc + Bp * mt
    if D1 != 0 or every:
        out = out + scaled_diff(D1, h[0], mt)
    if (D2 != 0 or every) and order >= 2:
        out = out + scaled_diff(D2, h[1], mt)
    return out, xc, torch.stack([mt] + [hist[j] for j in range(order - 1)])


class UniPCEmulator(MultistepEmulator):
    def mi355x_sd_unipc_update(self, x, eu, et, last, hist, order, out, coef, gs, gr, batch, per_sample, stream):
        assert order in (1, 2, 3) and coef % 16 == 0
        v = self.step_args(FORMS["unipc"], dict(x=x, eu=eu, et=et, last=last, hist=hist, out=out, coef=coef), batch, per_sample,
                           et and gr > 0, order)
        H = v["hist"].reshape(order, batch, per_sample)
        o, xc, Hn = emulate(v["x"], v["eu"], v["et"], v["last"], H, v["coef"], gs, gr if et else 0.0, order)
        v["last"].copy_(xc)   # (before out: at corr == 0 x_c IS x's memory, which out may be)
        v["out"].copy_(o)
        H.copy_(Hn)
        return 0
