"""tests/abi_emulator.py's Emulator with the two InstructPix2Pix entry points (ABI 24) and the step tails a loop test runs behind them
-- TEST INFRASTRUCTURE ONLY, like its bases.

guidance3_math() restates csrc/ip2p.hip in torch fp32, one rounding per operation and in the kernel's order: the combine
c = fma(gs, t - i, fma(gi, i - u, u)), the predicted originals fma(-sigma, e, x) of the x0 form, and the statistics of
tests/abi_emulator_guidance.py (two passes, the kernel's tree). refused() is the argument rule of both entries, read from
paddlemix_amd/ip2p_forms.py: what csrc/capi.hip span_entry refuses. Every call is recorded with copies of what it read and wrote."""
import torch

from paddlemix_amd.ip2p_forms import ENTRIES
from tests.abi_emulator import _flat
from tests.abi_emulator_ancestral import AncestralEmulator
from tests.abi_emulator_guidance import F32, tree_sum
from tests.abi_emulator_heun import HeunEmulator
from tests.abi_emulator_multistep import MultistepEmulator

INT64_MAX = 2 ** 63 - 1


def refused(entry, a):
    """the reason the row refuses the call with arguments `a` (by name), or None"""
    used = {k: entry.used.get(k, lambda _: True)(a) for k in entry.spans}
    for k in entry.spans:
        if used[k] and not a[k] and k not in entry.optional:
            return f"null pointer ({k})"
    if any(a[k] < 1 for k in entry.positive) or (entry.entry == "guidance3" and a["guidance_rescale"] > 0.0 and a["per_sample"] < 2):
        return "range"
    size = {k: f(a) for k, f in entry.spans.items()}
    if 4 * max(size.values()) > INT64_MAX:
        return "range"
    for w in entry.written:
        for r in entry.spans:
            if r != w and used[r] and a[r] and a[w] < a[r] + 4 * size[r] and a[r] < a[w] + 4 * size[w]:
                return f"{w} must not overlap {r}"
    return None


def _fma(a, b, c):
    """fl(a * b + c) on fp32 tensors: the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).to(F32)


def mix3(t, i, u, gs, gi):
    gs, gi = torch.tensor(gs, dtype=F32), torch.tensor(gi, dtype=F32)
    return _fma(gs, t - i, _fma(gi, i - u, u))


def guidance3_math(eps, gs, gi, gr=0.0, x=None, sigma=None):
    """eps fp32 [3, batch, n]; x fp32 [batch, n] and sigma (fp32 scalar tensor) for the x0 form -> fp32 [batch, n]"""
    t, i, u = eps
    x0 = gr > 0.0 and x is not None
    if x0:
        nsig = -sigma.to(F32)
        t, i, u = _fma(nsig, t, x), _fma(nsig, i, x), _fma(nsig, u, x)
    c = mix3(t, i, u, gs, gi)
    if gr > 0.0:
        n = c.shape[1]
        gr, one = torch.tensor(gr, dtype=F32), torch.tensor(1.0, dtype=F32)
        inv_n, inv_nm1 = one / torch.tensor(float(n), dtype=F32), one / torch.tensor(float(n - 1), dtype=F32)
        q = []
        for v in (t, c):
            d = v - (tree_sum(v) * inv_n)[:, None]
            q.append(tree_sum(d * d))
        r = torch.sqrt(q[0] * inv_nm1) / torch.sqrt(q[1] * inv_nm1)
        c = c * (gr * r + (one - gr))[:, None]
        if x0:
            c = (c - x) / nsig
    return c


class Ip2pEmulator(AncestralEmulator, MultistepEmulator, HeunEmulator):
    def __init__(self):
        super().__init__()
        self.guidance3_calls, self.ip2p_input_calls = [], []

    def mi355x_sd_guidance3(self, eps, x, coef, out, gs, gi, gr, batch, per_sample, stream):
        a = dict(eps=eps, x=x, coef=coef, out=out, guidance_scale=gs, image_guidance_scale=gi, guidance_rescale=gr, batch=batch,
                 per_sample=per_sample)
        assert refused(ENTRIES["guidance3"], a) is None, refused(ENTRIES["guidance3"], a)
        self.calls.append("guidance3")
        e = _flat(eps, 3 * batch * per_sample, F32).reshape(3, batch, per_sample)
        x0 = gr > 0.0 and bool(x)
        xv = _flat(x, batch * per_sample, F32).reshape(batch, per_sample) if x0 else None
        sigma = _flat(coef, 1, F32)[0] if x0 else None
        res = guidance3_math(e, gs, gi, gr, xv, sigma)
        _flat(out, batch * per_sample, F32).reshape(batch, per_sample).copy_(res)
        self.guidance3_calls.append(dict(eps=e.clone(), x=None if xv is None else xv.clone(), coef=coef, out=res.clone(), gs=gs, gi=gi,
                                         gr=gr, sigma=None if sigma is None else float(sigma)))
        return 0

    def mi355x_sd_ip2p_input(self, x, image_latents, out, scale, groups, batch, c_lat, c_img, hw, stream):
        a = dict(x=x, image_latents=image_latents, out=out, scale=scale, groups=groups, batch=batch, c_lat=c_lat, c_img=c_img, hw=hw)
        assert refused(ENTRIES["ip2p_input"], a) is None and groups * batch <= 65535, refused(ENTRIES["ip2p_input"], a)
        self.calls.append("ip2p_input")
        xv = _flat(x, batch * c_lat * hw, F32).reshape(1, batch, c_lat, hw)
        img = _flat(image_latents, groups * batch * c_img * hw, F32).reshape(groups, batch, c_img, hw)
        o = _flat(out, groups * batch * (c_lat + c_img) * hw, F32).reshape(groups, batch, c_lat + c_img, hw)
        o[:, :, :c_lat] = xv * torch.tensor(scale, dtype=F32)
        o[:, :, c_lat:] = img
        self.ip2p_input_calls.append(dict(scale=scale, groups=groups, batch=batch, c_lat=c_lat, c_img=c_img, hw=hw, out=o.clone()))
        return 0
