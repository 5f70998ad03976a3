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
from tests.step_forms import FORMS

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


def guided(eu, et, gs, gr, variance="two_pass", always=False):
    """the guided (and rescaled) model output every step form starts from: eu, et (or None: no guidance) fp32 [batch, n] -> e fp32.
    The rescale runs at gr > 0 (always: whatever gr is, as cfg_rescale_axpby's kernel does)"""
    if et is None:
        return eu
    n = eu.shape[1]
    gs, gr = torch.tensor(gs, dtype=F32), torch.tensor(gr, dtype=F32)
    one = torch.tensor(1.0, dtype=F32)
    e = (eu.double() + gs.double() * (et - eu).double()).to(F32)   # fma(gs, fl(t - u), u): one rounding after the exact product
    if gr > 0 or always:
        inv_n, inv_nm1 = one / torch.tensor(float(n), dtype=F32), one / torch.tensor(float(n - 1), dtype=F32)
        q = []
        for v in (et, e):
            s = tree_sum(v)
            if variance == "one_pass":
                q.append(tree_sum(v * v) - (s * inv_n) * s)
            else:
                d = v - (s * inv_n)[:, None]
                q.append(tree_sum(d * d))
        r = torch.sqrt(q[0] * inv_nm1) / torch.sqrt(q[1] * inv_nm1)
        e = e * (gr * r + (one - gr))[:, None]
    return e


def emulate(x, eu, et, coef, gs, gr, variance="two_pass"):
    """x, eu, et fp32 [batch, n]; coef fp32 (a, b) -> fp32 [batch, n]"""
    return coef[0] * x + coef[1] * guided(eu, et, gs, gr, variance, always=True)


class GuidanceEmulator(Emulator):
    def step_args(self, form, ptr, batch, per_sample, rescale, order=None):
        """The argument rule of the step-tail entries, asserted once for all of them: what check_step_args of csrc/capi.hip refuses.
        ptr: the pointers by operand name (tests/step_forms.py). No null but an optional operand; batch > 0 and per_sample >= 1
        (>= 2 with the rescale); a written span overlaps no other written span and nothing read, unless the two are a pair of
        form.same and one pointer. -> the operands as fp32 views of the memory, [planes,] batch, per_sample (None for a null; coef
        flat): a plane the launch writes is written through its view."""
        self.calls.append(form.entry)
        assert all(p or k in form.optional for k, p in ptr.items()), "null pointer"
        assert batch > 0 and per_sample >= (2 if rescale else 1)
        planes = {k: form.written.get(k, 1) or order for k in ptr}
        size = {k: form.width if k == "coef" else planes[k] * batch * per_sample for k in ptr}
        for i, w in enumerate(form.written):
            for r in list(form.written)[i + 1:] + [k for k in ptr if k not in form.written]:
                apart = not ptr[r] or ptr[w] + 4 * size[w] <= ptr[r] or ptr[r] + 4 * size[r] <= ptr[w]
                assert apart or ((w, r) in form.same and ptr[w] == ptr[r]), (w, r)
        return {k: None if not p else _flat(p, size[k], F32) if k == "coef" else
                _flat(p, size[k], F32).reshape(((planes[k],) if form.written.get(k, 1) != 1 else ()) + (batch, per_sample))
                for k, p in ptr.items()}

    def mi355x_sd_cfg_rescale_axpby(self, x, eu, et, out, coef, gs, gr, batch, per_sample, stream):
        assert coef   # (its two floats are outside the overlap rule of this entry)
        v = self.step_args(FORMS["guidance"], dict(x=x, eu=eu, et=et, out=out), batch, per_sample, True)
        v["out"].copy_(emulate(v["x"], v["eu"], v["et"], _flat(coef, 2, F32), gs, gr))
        return 0
