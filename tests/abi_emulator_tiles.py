"""The two tiled-VAE entry points of include/mi355x_sd.h (mi355x_sd_tile_gather, mi355x_sd_tile_blend) on host memory -- TEST
INFRASTRUCTURE ONLY, used as ``on_emulator(AutoencoderKL, cfg, P, backend=TileEmulator())``.

The blend is written the way the device kernel is specified -- the closed form per output element over at most four decoded tiles,
through the table of tile pointers and the stride arguments -- and NOT as the reference's sequential in-place loop: that loop is
tests/tiled_vae_ref.py, the thing the product is compared against."""
from __future__ import annotations

import ctypes

import torch

from tests.abi_emulator import Emulator, _flat


def _axis(N, S, lim, ext):
    """per output coordinate: tile index, coordinate in it, its extent, the previous tile's extent, the blend extent (0 outside
    the band) and the coordinate the blend reads in the previous tile"""
    P = torch.arange(N)
    i = P // lim
    p = P - i * lim
    E = torch.clamp(N - i * lim, max=S)
    Ep = torch.clamp(N - (i - 1) * lim, max=S)
    e = torch.minimum(torch.minimum(Ep, E), torch.tensor(ext))
    e = torch.where((i > 0) & (p < e), e, torch.zeros_like(e))
    q = Ep - e + p
    return i, p, E, Ep, e, q


class TileEmulator(Emulator):
    def mi355x_sd_tile_gather(self, src, B, C, H, W, y0, x0, sy, sx, ny, nx, wh, ww, first, count, dst, stream):
        self.calls.append("tile_gather")
        assert y0 + (ny - 1) * sy + wh <= H and x0 + (nx - 1) * sx + ww <= W and 0 <= first and first + count <= B * ny * nx
        s = _flat(src, B * C * H * W, torch.float32).reshape(B, C, H, W)
        d = _flat(dst, count * C * wh * ww, torch.float32).reshape(count, C, wh, ww)
        for n in range(first, first + count):
            b, t = divmod(n, ny * nx)
            iy, ix = divmod(t, nx)
            d[n - first].copy_(s[b, :, y0 + iy * sy:y0 + iy * sy + wh, x0 + ix * sx:x0 + ix * sx + ww])
        return 0

    def mi355x_sd_tile_blend(self, tile_ptrs, B, C, H, W, S, lim, ext, ny, nx, t_scp, t_sc, t_sx, out, o_sb, o_sc, o_sy, o_sx, stream):
        self.calls.append("tile_blend")
        assert 0 <= ext <= lim <= S and ny == -(-H // lim) and nx == -(-W // lim)
        table = torch.frombuffer((ctypes.c_char * (8 * B * ny * nx)).from_address(tile_ptrs), dtype=torch.int64,
                                 count=B * ny * nx).reshape(B, ny, nx).tolist()
        iy, py, Ey, Epy, ey, qy = [t[:, None] for t in _axis(H, S, lim, ext)]
        ix, px, Ex, Epx, ex, qx = [t[None, :] for t in _axis(W, S, lim, ext)]
        f32 = lambda t: t.to(torch.float64).to(torch.float32)  # noqa: E731
        wy = py.double() / ey.clamp(min=1).double()
        wx = px.double() / ex.clamp(min=1).double()
        wy0, wy1, wx0, wx1 = f32(1.0 - wy), f32(wy), f32(1.0 - wx), f32(wx)
        inv, inh = (ey > 0).expand(H, W), (ex > 0).expand(H, W)
        o = _flat(out, (B - 1) * o_sb + (C - 1) * o_sc + (H - 1) * o_sy + (W - 1) * o_sx + 1, torch.float32)
        for b in range(B):
            tiles = {}
            for i in range(ny):
                for j in range(nx):
                    eh, ew = min(S, H - i * lim), min(S, W - j * lim)
                    n = (C - 1) * (t_scp * eh * ew + t_sc) + (eh * ew - 1) * t_sx + 1
                    tiles[i, j] = _flat(table[b][i][j], n, torch.float32).as_strided(
                        (C, eh, ew), (t_scp * eh * ew + t_sc, ew * t_sx, t_sx))

            def fetch(di, dj, yy, xx):   # [C, H, W]: element (yy, xx) of tile (iy - di, ix - dj), zeros where there is none
                r = torch.zeros(C, H, W)
                for (i, j), t in tiles.items():
                    m = ((iy - di) == i) & ((ix - dj) == j)
                    if di:
                        m = m & (ey > 0)
                    if dj:
                        m = m & (ex > 0)
                    m = m.expand(H, W)
                    if m.any():
                        ys, xs = yy.expand(H, W)[m], xx.expand(H, W)[m]
                        r[:, m] = t[:, ys, xs]
                return r

            cur, tr, bl, tl = fetch(0, 0, py, px), fetch(1, 0, qy, px), fetch(0, 1, py, qx), fetch(1, 1, qy, qx)
            top = torch.where(inh, tl * wx0 + tr * wx1, tr)
            v = torch.where(inv, top * wy0 + cur * wy1, cur)
            left = torch.where(inv, tl * wy0 + bl * wy1, bl)
            res = torch.where(inh, left * wx0 + v * wx1, v)
            o[b * o_sb:].as_strided((C, H, W), (o_sc, o_sy, o_sx)).copy_(res)
        return 0
