"""mi355x_sd_plms_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=PlmsEmulator())``.

emulate() restates the device kernels (csrc/step_tail.hip PlmsStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the guided (and rescaled) model output is guided() of tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_plms_bounds.py:
  "swap_h12"         the planes of h1 and h2 exchanged
  "from_x"           the averaging row (from_park) starts from x instead of the parked sample
  "append_avg"       the averaging row stores e in the ring, as every other row does
  "convert_x"        the v-prediction conversion taken with x instead of S (differs on the averaging row)
  "drop_w3"          the fourth term left out
  "store_converted"  the ring takes the converted output instead of e
  "mul_nan"          every term and both of x and P are formed, with a zero weight where the row does not use them"""
from __future__ import annotations

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.plms_bounds import flags
from tests.step_forms import FORMS


def emulate(x, eu, et, P, H, coef, gs, gr, fault=None):
    """x, eu, et (or None), P fp32 [batch, n]; H fp32 [3, batch, n]; coef fp32, 12 values -> (out, P, H) fp32: the state as the
    launch leaves it (new tensors)"""
    a, b, p, q, w0, w1, w2, w3 = coef.to(F32)[:8]
    slot, park, from_park = flags(coef)
    e = guided(eu, et, gs, gr)
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
        v = self.step_args(FORMS["plms"], dict(x=x, eu=eu, et=et, P=park, H=hist, out=out, coef=coef), batch, per_sample, et and gr > 0)
        o, P, Hn = emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], gs, gr if et else 0.0)
        slot, parks, from_park = flags(v["coef"])
        if not from_park:   # only what the kernel writes is written: the other planes keep whatever they hold
            v["H"][slot].copy_(Hn[slot])
        if parks:
            v["P"].copy_(P)
        v["out"].copy_(o)
        return 0
