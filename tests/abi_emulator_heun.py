"""mi355x_sd_heun_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=HeunEmulator())``.

emulate() restates the device kernels (csrc/step_tail.hip HeunStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_heun_bounds.py: "from_x" (stage 2 starts from x instead of the parked sample), "mul_nan" (the terms
over state a stage must not read are formed with a zero weight instead of skipped: stage 1 adds 0 * S + 0 * D, stage 2 at g == 0
forms g * D), "bf16_deriv" (the parked derivative rounded to bfloat16 before use)."""
from __future__ import annotations

import torch

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.step_forms import FORMS


def emulate(x, eu, et, S, D, coef, gs, gr, fault=None):
    """x, eu, et (or None), S, D fp32 [batch, n]; coef fp32 (p, q, h, g, second) -> (out, S, D) fp32 [batch, n]: the planes as the
    launch leaves them (stage 1: new ones; stage 2: the very tensors passed in)"""
    p, q, h, g, second = coef.to(F32)
    e = guided(eu, et, gs, gr)
    d = p * x + q * e if p != 0 else q * e
    if second == 0:
        out = x + h * d
        if fault == "mul_nan":
            out = out + 0.0 * S + 0.0 * D
        return out, x.clone(), d
    if g != 0 or fault == "mul_nan":
        m = g * (D.to(torch.bfloat16).to(F32) if fault == "bf16_deriv" else D) + d
    else:
        m = d
    return (x if fault == "from_x" else S) + h * m, S, D


class HeunEmulator(GuidanceEmulator):
    def mi355x_sd_heun_update(self, x, eu, et, sample, deriv, out, coef, gs, gr, batch, per_sample, stream):
        v = self.step_args(FORMS["heun"], dict(x=x, eu=eu, et=et, S=sample, D=deriv, out=out, coef=coef), batch, per_sample, et and gr > 0)
        o, S, D = emulate(v["x"], v["eu"], v["et"], v["S"], v["D"], v["coef"], gs, gr if et else 0.0)
        if v["coef"][4] == 0:
            v["S"].copy_(S)
            v["D"].copy_(D)
        v["out"].copy_(o)
        return 0
