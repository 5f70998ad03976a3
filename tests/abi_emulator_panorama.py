"""tests/abi_emulator_sega.py's SegaEmulator with the two panorama entry points (ABI 26) and the PLMS tail a loop test runs behind
them -- TEST INFRASTRUCTURE ONLY, like its bases.

view_input_math() and view_merge_math() restate csrc/panorama.hip in torch fp32 by the kernels' element rule, not by the reference's
slices: an index table of the geometry (view v = iy * nx + ix at row iy * stride, column (ix * stride + j) mod W) gathers the input;
the merge visits the views in ascending v and adds each to a sum that starts at +0.0 only where the view covers, then divides by the
number of covering views (a float32 division; the sum itself where none covers). refused() is the argument rule of both entries,
read from paddlemix_amd/panorama_forms.py: what csrc/capi.hip refuses. Every call is recorded."""
import torch

from paddlemix_amd import panorama_forms as PF
from tests.abi_emulator import _flat
from tests.abi_emulator_guidance import F32
from tests.abi_emulator_plms import PlmsEmulator
from tests.abi_emulator_sega import SegaEmulator

ENTRIES = PF.ENTRIES
GEOMETRY = ("batch", "C", "H", "W", "win_h", "win_w", "stride", "ny", "nx", "circular")


def refused(entry, a):
    """the reason the row refuses the call with arguments `a` (by name), or None; "unsupported" is the launcher's own refusal"""
    for k in entry.spans:
        if not a[k]:
            return f"null pointer ({k})"
    if entry.entry == "view_input" and a["groups"] not in (1, 2):
        return "groups"
    bad = PF.geometry_rule(a)
    if bad:
        return bad
    if entry.entry == "view_input":
        if a["first"] < 0 or a["count"] < 0 or a["first"] + a["count"] > a["ny"] * a["nx"]:
            return "first, count"
        if 4 * entry.spans["out"](a) > PF.INT64_MAX:
            return "count"
    size = {k: f(a) for k, f in entry.spans.items()}
    for w in entry.written:
        for r in entry.spans:
            if r != w and a[w] < a[r] + 4 * size[r] and a[r] < a[w] + 4 * size[w]:
                return f"{w} must not overlap {r}"
    planes = (a["count"] if entry.entry == "view_input" else 1) * a["batch"] * a["C"]
    rows = a["win_h"] if entry.entry == "view_input" else a["H"]
    if planes > PF.MAX_PLANES or (rows + 3) // 4 > 65535:
        return "unsupported"
    return None


def columns(W, win_w, stride, nx, circular):
    """[nx, win_w] source column of every view column"""
    col = torch.arange(nx)[:, None] * stride + torch.arange(win_w)[None, :]
    return col % W if circular else col


def view_input_math(x, scale, groups, win_h, win_w, stride, ny, nx, circular, first, count):
    """x fp32 [B, C, H, W] -> [groups, count * B, C, win_h, win_w]"""
    B, C, H, W = x.shape
    col = columns(W, win_w, stride, nx, circular)
    out = []
    for v in range(first, first + count):
        iy, ix = divmod(v, nx)
        out.append(x[:, :, iy * stride:iy * stride + win_h][:, :, :, col[ix]])
    one = torch.cat(out) * torch.tensor(scale, dtype=F32) if out else x.new_zeros((0, C, win_h, win_w))
    return torch.stack([one] * groups)


def view_merge_math(views, B, C, H, W, win_h, win_w, stride, ny, nx, circular):
    """views fp32 [ny * nx * B, C, win_h, win_w] -> [B, C, H, W]"""
    col = columns(W, win_w, stride, nx, circular)
    total = torch.zeros(B, C, H, W, dtype=F32)                    # +0.0f
    n = torch.zeros(H, W, dtype=torch.int32)
    for v in range(ny * nx):
        iy, ix = divmod(v, nx)
        placed = torch.zeros(B, C, H, W, dtype=F32)
        cover = torch.zeros(H, W, dtype=torch.bool)
        rows = slice(iy * stride, iy * stride + win_h)
        placed[:, :, rows, :].index_copy_(3, col[ix], views[v * B:(v + 1) * B])   # (a basic slice is a view: written in place)
        cover[rows, :].index_fill_(1, col[ix], True)
        total = torch.where(cover, total + placed, total)        # one fp32 addition per covered element, in view order
        n += cover.to(torch.int32)
    cnt = n.to(F32)
    return torch.where(n > 0, total / torch.where(n > 0, cnt, torch.ones_like(cnt)), total)


class PanoramaEmulator(SegaEmulator, PlmsEmulator):
    def __init__(self):
        super().__init__()
        self.view_input_calls, self.view_merge_calls = [], []

    def mi355x_sd_view_input(self, x, out, scale, groups, batch, C, H, W, win_h, win_w, stride, ny, nx, circular, first, count, stream):
        a = dict(x=x, out=out, scale=scale, groups=groups, batch=batch, C=C, H=H, W=W, win_h=win_h, win_w=win_w, stride=stride, ny=ny,
                 nx=nx, circular=circular, first=first, count=count)
        assert refused(ENTRIES["view_input"], a) is None, refused(ENTRIES["view_input"], a)
        self.calls.append("view_input")
        xv = _flat(x, batch * C * H * W, F32).reshape(batch, C, H, W)
        res = view_input_math(xv, scale, groups, win_h, win_w, stride, ny, nx, circular, first, count)
        _flat(out, res.numel(), F32).copy_(res.flatten())
        self.view_input_calls.append(dict(a, result=res.clone()))
        return 0

    def mi355x_sd_view_merge(self, views, out, batch, C, H, W, win_h, win_w, stride, ny, nx, circular, stream):
        a = dict(views=views, out=out, batch=batch, C=C, H=H, W=W, win_h=win_h, win_w=win_w, stride=stride, ny=ny, nx=nx,
                 circular=circular)
        assert refused(ENTRIES["view_merge"], a) is None, refused(ENTRIES["view_merge"], a)
        self.calls.append("view_merge")
        vv = _flat(views, ny * nx * batch * C * win_h * win_w, F32).reshape(ny * nx * batch, C, win_h, win_w)
        res = view_merge_math(vv, batch, C, H, W, win_h, win_w, stride, ny, nx, circular)
        _flat(out, res.numel(), F32).copy_(res.flatten())
        self.view_merge_calls.append(dict(a, result=res.clone()))
        return 0
