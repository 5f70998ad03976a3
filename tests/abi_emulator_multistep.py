"""mi355x_sd_multistep_update of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=MultistepEmulator())``.

emulate() restates the device kernels (csrc/misc.hip multistep_kernel / multistep_rescale_kernel) in torch fp32, one rounding per
operation and in the kernel's own order; the statistics of the rescale go through tree_sum of tests/abi_emulator_guidance.py. It is
NOT convert_model_output + scheduler.step: that is the generic loop the fused loop is compared against. ``fault`` restates a
FAULT for tests/test_multistep_bounds.py: "regroup" ((B + D) m0 - D m1), "mul_nan" (D * (m0 - m1) computed at D = 0 instead of
skipped), "one_pass" (the fp32 sum v^2 - n mean^2 variance)."""
from __future__ import annotations

import torch

from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32, GuidanceEmulator, tree_sum


def emulate(x, eu, et, m1, coef, gs, gr, fault=None):
    """x, eu, et (or None), m1 fp32 [batch, n]; coef fp32 (p, q, A, B, D) -> (out, m0) fp32 [batch, n]"""
    n = x.shape[1]
    p, q, A, B, D = coef.to(F32)
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
    m0 = p * x + q * e
    if fault == "regroup":
        return (A * x + (B + D) * m0) - D * m1, m0
    out = A * x + B * m0
    if D != 0 or fault == "mul_nan":
        out = out + D * (m0 - m1)
    return out, m0


class MultistepEmulator(GuidanceEmulator):
    def mi355x_sd_multistep_update(self, x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream):
        self.calls.append("multistep_update")
        assert x and eu and m_prev and out and m_out and coef and batch > 0 and per_sample >= (2 if et and gr > 0 else 1)
        n = batch * per_sample
        apart = lambda a, b: a + 4 * n <= b or b + 4 * n <= a  # noqa: E731
        assert apart(out, m_out) and (out == x or apart(out, x)) and (m_out == m_prev or apart(m_out, m_prev))
        assert apart(out, m_prev) and apart(m_out, x) and all(apart(w, p) for w in (out, m_out) for p in (eu, et) if p)
        v = [_flat(p, n, F32).reshape(batch, per_sample) if p else None for p in (x, eu, et, m_prev)]
        o, m0 = emulate(*v, _flat(coef, 5, F32), gs, gr)
        _flat(out, n, F32).copy_(o.reshape(-1))
        _flat(m_out, n, F32).copy_(m0.reshape(-1))
        return 0
