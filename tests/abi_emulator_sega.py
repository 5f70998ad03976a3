"""tests/abi_emulator_ip2p.py's Ip2pEmulator with mi355x_sd_sega_guidance (ABI 25) -- TEST INFRASTRUCTURE ONLY, like its bases.

sega_math() restates csrc/sega.hip in torch fp32, one rounding per operation and in the kernel's order. The selection is the
kernel's rule, not its algorithm: the order statistics lo and hi of the plane's |g| by a sort (a radix select and a sort name the same
element), the threshold by the kernel's one-fma lerp, NaN when the plane holds a NaN. refused() is the argument rule of the entry,
read from paddlemix_amd/sega_forms.py: what csrc/capi.hip span_entry refuses. Every call is recorded with copies of what it read and
wrote."""
import numpy as np
import torch

from paddlemix_amd import sega_forms as SF
from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32
from tests.abi_emulator_ip2p import INT64_MAX, Ip2pEmulator, _fma

ENTRY = SF.ENTRIES["sega_guidance"]


def refused(entry, a):
    """the reason the row refuses the call with arguments `a` (by name), or None; "unsupported" is the launcher's own refusal"""
    used = {k: entry.used.get(k, lambda _: True)(a) for k in entry.spans}
    for k in entry.spans:
        if used[k] and not a[k] and k not in entry.optional:
            return f"null pointer ({k})"
    if any(a[k] < 1 for k in entry.positive):
        return "range"
    size = {k: f(a) for k, f in entry.spans.items()}
    if 4 * max(size.values()) > INT64_MAX:
        return "range"
    for w in entry.written:
        for r in entry.spans:
            if r != w and used[w] and used[r] and a[w] and a[r] and a[w] < a[r] + 4 * size[r] and a[r] < a[w] + 4 * size[w]:
                return f"{w} must not overlap {r}"
    if a["n_concepts"] > SF.MAX_CONCEPTS or a["hw"] > SF.MAX_HW:
        return "unsupported"
    return None


def parse_row(row, n):
    """row: int32 / uint32 words (numpy) -> dict of the fields csrc/sega.hip reads"""
    w = np.ascontiguousarray(np.asarray(row)).view(np.uint32)[:SF.row_words(n)]
    f = w.view(np.float32)
    i = w.view(np.int32)
    at = [SF.ROW_HEAD + SF.ROW_PER * c for c in range(n)]
    per = [dict(scale=f[k], lo=int(i[k + 1]), frac=f[k + 2], w_full=f[k + 3], w_part=f[k + 4]) for k in at]
    return dict(regime=int(w[0]), active=int(w[1]), warm=int(w[2]), gs=f[4], ms=f[5], beta=f[6], omb=f[7], per=per)


def _t(v):
    return torch.tensor(float(v), dtype=F32)


def select(absg, lo, frac):
    """absg fp32 [planes, hw] -> (v[lo], v[hi], thr) fp32 [planes]: the kernel's rule"""
    hw = absg.shape[1]
    lo = min(max(lo, 0), hw - 1)
    hi = lo + 1 if (float(frac) != 0.0 and lo + 1 <= hw - 1) else lo
    keys = absg.contiguous().view(torch.int32)          # the bit patterns of non-negative floats order as integers, NaNs last
    order = torch.sort(keys, dim=1).values.view(F32)
    vlo, vhi = order[:, lo], order[:, hi]
    diff, w = vhi - vlo, _t(frac)
    thr = _fma(w, diff, vlo) if abs(float(frac)) < 0.5 else _fma(w - _t(1.0), diff, vhi)
    thr = torch.where(torch.isnan(absg).any(dim=1), torch.full_like(thr, float("nan")), thr)
    return vlo, vhi, thr


def sega_math(eps, momentum, extra, row, n):
    """eps fp32 [2 + n, batch, channels, hw]; momentum, extra fp32 [batch, channels, hw] -> (out, momentum', stats [n, batch, channels, 3])"""
    r = parse_row(row, n)
    u, t = eps[0], eps[1]
    B, C, hw = u.shape
    guid = _t(r["gs"]) * (t - u)
    edit, part = torch.zeros_like(u), torch.zeros_like(u)
    stats = torch.zeros(n, B, C, 3, dtype=F32)
    for c, pc in enumerate(r["per"]):
        g = torch.zeros_like(u)
        if (r["active"] >> c) & 1:
            d = (eps[2 + c] - u) * _t(pc["scale"])
            vlo, vhi, thr = select(d.abs().reshape(B * C, hw), pc["lo"], pc["frac"])
            stats[c] = torch.stack([vlo, vhi, thr], dim=1).reshape(B, C, 3)
            g = torch.where(d.abs() >= thr.reshape(B, C, 1), d, torch.zeros_like(d))
        edit = _fma(_t(pc["w_full"]), g, edit)
        if (r["warm"] >> c) & 1:
            part = _fma(_t(pc["w_part"]), g, part)
    if r["regime"] == SF.REGIME_PARTIAL:
        guid = guid + part
    edit = _fma(_t(r["ms"]), momentum, edit)
    mom = _fma(_t(r["beta"]), momentum, _t(r["omb"]) * edit)
    if r["regime"] == SF.REGIME_ALL:
        guid = guid + edit
    if extra is not None:
        guid = guid + extra
    return u + guid, mom, stats


class SegaEmulator(Ip2pEmulator):
    def __init__(self):
        super().__init__()
        self.sega_calls = []

    def mi355x_sd_sega_guidance(self, eps, momentum, extra, row, out, stats, n, batch, channels, hw, stream):
        a = dict(eps=eps, momentum=momentum, extra=extra, row=row, out=out, stats=stats, n_concepts=n, batch=batch, channels=channels, hw=hw)
        assert refused(ENTRY, a) is None, refused(ENTRY, a)
        self.calls.append("sega_guidance")
        plane = batch * channels * hw
        e = _flat(eps, (2 + n) * plane, F32).reshape(2 + n, batch, channels, hw)
        m = _flat(momentum, plane, F32).reshape(batch, channels, hw)
        x = _flat(extra, plane, F32).reshape(batch, channels, hw) if extra else None
        words = _flat(row, SF.row_words(n), F32).numpy().view(np.int32).copy()
        res, mom, st = sega_math(e, m, x, words, n)
        self.sega_calls.append(dict(eps=e.clone(), momentum=m.clone(), extra=None if x is None else x.clone(), row=words, row_ptr=row,
                                    out=res.clone(), momentum_out=mom.clone(), stats=st))
        m.copy_(mom)
        _flat(out, plane, F32).reshape(batch, channels, hw).copy_(res)
        if stats:
            _flat(stats, 3 * n * batch * channels, F32).copy_(st.flatten())
        return 0
