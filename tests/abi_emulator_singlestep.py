"""mi355x_sd_singlestep_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=SinglestepEmulator())``.

emulate() restates the device kernels (csrc/step_tail.hip SinglestepStep in step_flat_kernel / step_rescale_kernel) in torch fp32, one
rounding per operation and in the kernel's own order; the guided (and rescaled) model output is guided() of
tests/abi_emulator_guidance.py. It is NOT scheduler.step: that is the generic loop the fused loop is compared against. ``fault``
restates a FAULT for tests/test_singlestep_bounds.py:
  "regroup"       (B - E1 - E2) b + E1 m0 + E2 m1 instead of the differences against b
  "read_park_o1"  an order-1 row forms A S with S read from the parked sample whatever the order (and so over a fresh loop's NaN)
  "park_o2"       an order-2 row parks x as an order-1 row does
  "skip_keep"     the plane-1 store of an order-2 row with keep != 0 is left out
  "mul_nan"       the E2 term is formed on every row of order 2 and 3, with its zero coefficient where the row does not use plane 1"""
from __future__ import annotations

from tests.abi_emulator_guidance import F32, GuidanceEmulator, guided
from tests.singlestep_bounds import flags
from tests.step_forms import FORMS


def emulate(x, eu, et, P, H, coef, gs, gr, fault=None):
    """x, eu, et (or None), P fp32 [batch, n]; H fp32 [2, batch, n]; coef fp32, 8 values -> (out, P, H) fp32: the state as the launch
    leaves it (new tensors)"""
    p, q, A, B, E1, E2 = coef.to(F32)[:6]
    order, keep, heun = flags(coef)
    e = guided(eu, et, gs, gr)
    m0 = p * x + q * e
    if order == 1:
        out = A * (P if fault == "read_park_o1" else x) + B * m0
    elif fault == "regroup":
        out = A * P + (B - E1 - (E2 if heun else 0.0)) * H[0] + E1 * m0
        if heun:
            out = out + E2 * H[1]
    else:
        out = A * P + B * H[0] + E1 * (m0 - H[0])
        if heun or fault == "mul_nan":
            out = out + E2 * (H[1] - H[0])
    H, P = H.clone(), P.clone()
    if order == 1:
        P, H[0] = x.clone(), m0
    elif keep and fault != "skip_keep":
        H[1] = m0
    if order == 2 and fault == "park_o2":
        P = x.clone()
    return out, P, H


class SinglestepEmulator(GuidanceEmulator):
    def mi355x_sd_singlestep_update(self, x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream):
        v = self.step_args(FORMS["singlestep"], dict(x=x, eu=eu, et=et, P=park, H=hist, out=out, coef=coef), batch, per_sample, et and gr > 0)
        o, P, Hn = emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], gs, gr if et else 0.0)
        order, keep, _ = flags(v["coef"])
        if order == 1:   # only what the kernel writes is written: everything else keeps whatever it holds
            v["P"].copy_(P)
            v["H"][0].copy_(Hn[0])
        elif keep:
            v["H"][1].copy_(Hn[1])
        v["out"].copy_(o)
        return 0
