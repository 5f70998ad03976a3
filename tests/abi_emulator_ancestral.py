"""mi355x_sd_ancestral_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=AncestralEmulator())``.

emulate() restates the device kernels (csrc/misc.hip ancestral_kernel / ancestral_rescale_kernel) in torch fp32, one rounding per
operation and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is
NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault`` restates a FAULT for
tests/test_ancestral_bounds.py: "mul_nan" (c * z computed at c = 0 instead of skipped), "bf16_noise" (z rounded to bfloat16 before
use), "one_pass" (the fp32 sum v^2 - n mean^2 variance)."""
from __future__ import annotations

import torch

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.step_forms import FORMS


def emulate(x, eu, et, z, coef, gs, gr, fault=None):
    """x, eu, et (or None), z (or None at c = 0) fp32 [batch, n]; coef fp32 (a, b, c) -> out fp32 [batch, n]"""
    a, b, c = coef.to(F32)
    e = guided(eu, et, gs, gr, "one_pass" if fault == "one_pass" else "two_pass")
    out = a * x + b * e
    if c != 0 or fault == "mul_nan":
        out = out + c * (z.to(torch.bfloat16).to(F32) if fault == "bf16_noise" else z)
    return out


class AncestralEmulator(GuidanceEmulator):
    def mi355x_sd_ancestral_update(self, x, eu, et, noise, out, coef, gs, gr, batch, per_sample, stream):
        v = self.step_args(FORMS["ancestral"], dict(x=x, eu=eu, et=et, z=noise, out=out, coef=coef), batch, per_sample, et and gr > 0)
        assert noise or v["coef"][2] == 0, "a null noise plane on a row with c != 0"
        v["out"].copy_(emulate(v["x"], v["eu"], v["et"], v["z"], v["coef"], gs, gr if et else 0.0))
        return 0
