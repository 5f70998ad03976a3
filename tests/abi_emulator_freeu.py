"""tests/abi_emulator.py's Emulator with the FreeU entry points (ABI 22) -- TEST INFRASTRUCTURE ONLY, like its base.

``mi355x_sd_freeu`` on host memory, by the closed form the kernel evaluates (tests/freeu_bounds.closed_form, float64, one rounding to
the buffer's element type), not by an FFT: what tests/test_freeu_host.py then compares with the FFT-based oracle is the form too.
Every call is recorded in ``freeu_calls`` with its arguments, and "freeu" joins ``calls`` -- GroupNorm entries there are "gn_fused" /
"gn_stats", the ControlNet adds are recorded here as "add_nchw" -- so the placement of a launch can be read off the list."""
import math

import torch

from tests import freeu_bounds as FB
from tests.abi_emulator import Emulator, _rows


class FreeUEmulator(Emulator):
    def __init__(self):
        super().__init__()
        self.freeu_calls = []

    def mi355x_sd_add_nchw(self, *a, **k):
        self.calls.append("add_nchw")
        return super().mi355x_sd_add_nchw(*a, **k)

    def mi355x_sd_freeu_workspace_floats(self, B, H, W, Cs):
        return FB.workspace_floats(B, H, W, Cs)   # the library's own answer: a plan made here may be replayed on the device

    def mi355x_sd_freeu(self, cat, ld, B, H, W, Cx, Cs, b, s, elem_f32, workspace, stream):
        es = 4 if elem_f32 else 2
        # the refusals of the entry (include/mi355x_sd.h)
        assert cat and workspace and B >= 1 and H >= 2 and W >= 2 and Cx >= 0 and Cs >= 1 and ld >= Cx + Cs
        assert cat % 16 == 0 and (ld * es) % 16 == 0 and math.isfinite(b) and math.isfinite(s)
        self.calls.append("freeu")
        self.freeu_calls.append(dict(index=len(self.calls) - 1, ld=ld, B=B, H=H, W=W, Cx=Cx, Cs=Cs, b=b, s=s, elem_f32=elem_f32))
        rows = _rows(cat, B * H * W, Cx + Cs, ld, torch.float32 if elem_f32 else None)
        b, s = FB.fp32(b), FB.fp32(s)
        half = Cx // 2
        x = rows.double()
        rows[:, :half] = (x[:, :half] * b).to(rows.dtype)
        planes = x[:, Cx:].reshape(B, H, W, Cs).permute(0, 3, 1, 2)
        rows[:, Cx:] = FB.closed_form(planes, s).permute(0, 2, 3, 1).reshape(B * H * W, Cs).to(rows.dtype)
        return 0
