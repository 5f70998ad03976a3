"""mi355x_sd_multistep_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=MultistepEmulator())``.

emulate() restates the device kernels (csrc/misc.hip multistep_kernel / multistep_rescale_kernel) in torch fp32, one rounding per
operation and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is
NOT convert_model_output + scheduler.step: that is the generic loop the fused loop is compared against. ``fault`` restates a
FAULT for tests/test_multistep_bounds.py: "regroup" ((B + D) m0 - D m1), "mul_nan" (D * (m0 - m1) computed at D = 0 instead of
skipped), "one_pass" (the fp32 sum v^2 - n mean^2 variance)."""
from __future__ import annotations

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.step_forms import FORMS


def emulate(x, eu, et, m1, coef, gs, gr, fault=None):
    """x, eu, et (or None), m1 fp32 [batch, n]; coef fp32 (p, q, A, B, D) -> (out, m0) fp32 [batch, n]"""
    p, q, A, B, D = coef.to(F32)
    e = guided(eu, et, gs, gr, "one_pass" if fault == "one_pass" else "two_pass")
    m0 = p * x + q * e
    if fault == "regroup":
        return (A * x + (B + D) * m0) - D * m1, m0
    out = A * x + B * m0
    if D != 0 or fault == "mul_nan":
        out = out + D * (m0 - m1)
    return out, m0


class MultistepEmulator(GuidanceEmulator):
    def mi355x_sd_multistep_update(self, x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream):
        v = self.step_args(FORMS["multistep"], dict(x=x, eu=eu, et=et, m1=m_prev, out=out, m_out=m_out, coef=coef), batch, per_sample,
                           et and gr > 0)
        o, m0 = emulate(v["x"], v["eu"], v["et"], v["m1"], v["coef"], gs, gr)
        v["out"].copy_(o)
        v["m_out"].copy_(m0)
        return 0
