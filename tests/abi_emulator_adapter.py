"""tests/abi_emulator.py's Emulator with the T2I-Adapter entry points (ABI 23) -- TEST INFRASTRUCTURE ONLY, like its base.

``mi355x_sd_pixel_unshuffle``, ``mi355x_sd_avgpool2`` and ``mi355x_sd_relu`` on host memory in torch, with the refusals of the entries
(include/mi355x_sd.h) as assertions and the device's rounding points: fp32 arithmetic, one rounding to the buffer's element type.
``mi355x_sd_add_nchw`` / ``_ex`` are recorded in ``calls`` as "add_nchw" (the base records neither), and the three new entries under
their own names."""
import torch
import torch.nn.functional as F

from paddlemix_amd import _lib
from tests.abi_emulator import Emulator, _flat, _rows


class AdapterEmulator(Emulator):
    def mi355x_sd_add_nchw(self, *a, **k):
        self.calls.append("add_nchw")
        return super().mi355x_sd_add_nchw(*a, **k)

    def mi355x_sd_pixel_unshuffle(self, x, B, C, H, W, r, y, ldy, stream):
        assert x and y and min(B, C, H, W, r) >= 1 and H % r == 0 and W % r == 0 and ldy >= C * r * r and ldy % 8 == 0 and y % 16 == 0
        self.calls.append("pixel_unshuffle")
        xs = _flat(x, B * C * H * W, torch.float32).reshape(B, C, H, W)
        rows = F.pixel_unshuffle(xs, r).permute(0, 2, 3, 1).reshape(B * (H // r) * (W // r), C * r * r)
        _rows(y, rows.shape[0], rows.shape[1], ldy).copy_(rows.to(_lib.elem_dtype()))
        return 0

    def mi355x_sd_avgpool2(self, x, ldx, B, H, W, C, y, ldy, stream):
        assert x and y and min(B, H, W, C) >= 1 and ldx >= C and ldy >= C
        assert C % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0 and x % 16 == 0 and y % 16 == 0
        self.calls.append("avgpool2")
        xs = _rows(x, B * H * W, C, ldx).float().reshape(B, H, W, C).permute(0, 3, 1, 2)
        o = F.avg_pool2d(xs, 2, 2, ceil_mode=True, count_include_pad=False)
        Ho, Wo = o.shape[2], o.shape[3]
        assert (Ho, Wo) == ((H + 1) // 2, (W + 1) // 2)
        _rows(y, B * Ho * Wo, C, ldy).copy_(o.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C).to(_lib.elem_dtype()))
        return 0

    def mi355x_sd_relu(self, x, ldx, y, ldy, rows, C, stream):
        assert x and y and rows >= 1 and C >= 1 and ldx >= C and ldy >= C
        self.calls.append("relu")
        _rows(y, rows, C, ldy).copy_(torch.relu(_rows(x, rows, C, ldx).clone()))
        return 0
