"""mi355x_sd_dpm2_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=Dpm2Emulator())``.

emulate() restates the device kernels (csrc/step_tail.hip MidpointStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_dpm2_bounds.py: "from_x" (stage 2 starts from x instead of the parked sample), "mul_nan" (the terms
over state a row must not read are formed with a zero weight instead of skipped: stage 1 adds 0 * S, every row at c == 0 or in stage 1
adds c * z), "bf16_noise" (the noise rounded to bfloat16 before use)."""
from __future__ import annotations

import torch

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.step_forms import FORMS


def emulate(x, eu, et, z, S, coef, gs, gr, fault=None):
    """x, eu, et (or None), z (or None where the row reads none), S fp32 [batch, n]; coef fp32 (p, q, h, c, second) -> (out, S) fp32
    [batch, n]: the plane as the launch leaves it (stage 1: a new one; stage 2: the very tensor passed in)"""
    p, q, h, c, second = coef.to(F32)
    e = guided(eu, et, gs, gr)
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
        v = self.step_args(FORMS["dpm2"], dict(x=x, eu=eu, et=et, z=noise, S=sample, out=out, coef=coef), batch, per_sample, et and gr > 0)
        k = v["coef"]
        assert noise or k[4] == 0 or k[3] == 0        # a null plane only where the row reads none
        o, S = emulate(v["x"], v["eu"], v["et"], v["z"], v["S"], k, gs, gr if et else 0.0)
        if k[4] == 0:
            v["S"].copy_(S)
        v["out"].copy_(o)
        return 0
