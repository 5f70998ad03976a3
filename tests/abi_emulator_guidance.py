"""mi355x_sd_cfg_rescale_axpby of include/mi355x_sd.h on host memory -- TEST INFRASTRUCTURE ONLY, used as
``on_emulator(UNet2DConditionModel, cfg, P, backend=GuidanceEmulator())``.

emulate() restates the device kernel (csrc/misc.hip cfg_rescale_axpby_kernel) in torch fp32, one rounding per operation and in the
kernel's own order: the mean first, then the squared deviations from it, every sum through the kernel's tree (a lane's elements
tid, tid + 1024, ... in order, a 64-lane butterfly, a 16-partial butterfly). It is NOT rescale_noise_cfg + scheduler.step: that
is the generic loop of paddlemix_amd/pipeline.py, the thing the fused loop is compared against. ``variance="one_pass"`` restates
a FAULT, the fp32 sum v^2 - n mean^2 form, for tests/test_guidance_bounds.py."""
from __future__ import annotations

import torch

from tests.abi_emulator import Emulator, _flat

F32 = torch.float32
THREADS = 1024


def tree_sum(v):
    """v fp32 [batch, n] -> [batch]: the kernel's reduction order (adding the 0 of an idle lane changes nothing)"""
    batch, n = v.shape
    trips = (n + THREADS - 1) // THREADS
    p = torch.zeros(batch, trips * THREADS, dtype=F32)
    p[:, :n] = v
    p = p.reshape(batch, trips, THREADS)
    s = torch.zeros(batch, THREADS, dtype=F32)
    for j in range(trips):
        s = s + p[:, j]
    s = s.reshape(batch, THREADS // 64, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ o]
    w = s[..., 0]
    parts = torch.arange(THREADS // 64)
    for o in (8, 4, 2, 1):
        w = w + w[..., parts ^ o]
    return w[:, 0]


def emulate(x, eu, et, coef, gs, gr, variance="two_pass"):
    """x, eu, et fp32 [batch, n]; coef fp32 (a, b) -> fp32 [batch, n]"""
    n = x.shape[1]
    gs, gr = torch.tensor(gs, dtype=F32), torch.tensor(gr, dtype=F32)
    one = torch.tensor(1.0, dtype=F32)
    c = (eu.double() + gs.double() * (et - eu).double()).to(F32)   # fma(gs, fl(t - u), u): one rounding after the exact product
    inv_n, inv_nm1 = one / torch.tensor(float(n), dtype=F32), one / torch.tensor(float(n - 1), dtype=F32)
    q = []
    for v in (et, c):
        s = tree_sum(v)
        if variance == "one_pass":
            q.append(tree_sum(v * v) - (s * inv_n) * s)
        else:
            d = v - (s * inv_n)[:, None]
            q.append(tree_sum(d * d))
    r = torch.sqrt(q[0] * inv_nm1) / torch.sqrt(q[1] * inv_nm1)
    k = gr * r + (one - gr)
    return coef[0] * x + coef[1] * (c * k[:, None])


class GuidanceEmulator(Emulator):
    def mi355x_sd_cfg_rescale_axpby(self, x, eu, et, out, coef, gs, gr, batch, per_sample, stream):
        self.calls.append("cfg_rescale_axpby")
        assert batch > 0 and per_sample >= 2
        n = batch * per_sample
        assert out == x or out + 4 * n <= x or x + 4 * n <= out
        assert all(out + 4 * n <= p or p + 4 * n <= out for p in (eu, et))
        v = [_flat(p, n, F32).reshape(batch, per_sample) for p in (x, eu, et)]
        _flat(out, n, F32).copy_(emulate(*v, _flat(coef, 2, F32), gs, gr).reshape(-1))
        return 0
