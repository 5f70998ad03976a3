"""Torch restatement of the reference's tiled VAE (AutoencoderKL.tiled_decode / tiled_encode with blend_v / blend_h,
PPD/models/autoencoder_kl.py:334-446) on top of the oracle's untiled decoder / encoder -- TEST INFRASTRUCTURE ONLY.

``blend_tiles`` is the reference's second loop as written there: sequential, in place, a later tile reading its neighbours after
their own blends. ``blend_closed_form64`` evaluates the closed form the device kernel implements in float64, together with the
magnitude sum(w_k * |D_k|) of each output element that scales its rounding bound."""
from __future__ import annotations

import torch

from oracle import vae_ref as R


def _blend(prev, tile, extent, dim):
    """in place: the first e = min(both extents, extent) rows (dim 2) / columns (dim 3) of `tile` become a ramp from the last e of
    `prev` to themselves; the weights are Python floats (double) that meet the fp32 tensor as fp32, as in the reference"""
    e = min(prev.shape[dim], tile.shape[dim], extent)
    w = torch.arange(e, dtype=torch.float64) / max(e, 1)
    shape = [1, 1, 1, 1]
    shape[dim] = e
    w0, w1 = (1 - w).to(tile.dtype).reshape(shape), w.to(tile.dtype).reshape(shape)
    head = tile.narrow(dim, 0, e)
    head.copy_(prev.narrow(dim, prev.shape[dim] - e, e) * w0 + head * w1)
    return tile


def blend_tiles(rows, blend_extent, row_limit, blend=True):
    """rows[i][j]: [B, C, eh, ew] as decoded (left untouched: the in-place sequence runs on copies). Row-major: a tile is blended
    with the FINISHED tile above, then with the FINISHED tile to its left, then cropped; crops are joined."""
    done = [[t.clone() for t in row] for row in rows]
    bands = []
    for i, row in enumerate(done):
        for j, tile in enumerate(row):
            if blend and i:
                _blend(done[i - 1][j], tile, blend_extent, 2)
            if blend and j:
                _blend(row[j - 1], tile, blend_extent, 3)
        bands.append(torch.cat([t[:, :, :row_limit, :row_limit] for t in row], dim=3))
    return torch.cat(bands, dim=2)


def split(x, size, stride):
    return [[x[:, :, i:i + size, j:j + size] for j in range(0, x.shape[3], stride)] for i in range(0, x.shape[2], stride)]


def tiled_decode(P, cfg, z, T, S, f=0.25, scaled=False, blend=True):
    overlap_size, blend_extent = int(T * (1 - f)), int(S * f)
    rows = [[R.decode(P, cfg, t, scaled=scaled) for t in row] for row in split(z, T, overlap_size)]
    return blend_tiles(rows, blend_extent, S - blend_extent, blend)


def tiled_encode_moments(P, cfg, x, T, S, f=0.25):
    overlap_size, blend_extent = int(S * (1 - f)), int(T * f)
    rows = [[R.encode_moments(P, cfg, t) for t in row] for row in split(x, S, overlap_size)]
    return blend_tiles(rows, blend_extent, T - blend_extent)


def tiled_encode(P, cfg, x, T, S, f=0.25, noise=None):
    """-> (mean, logvar, sample) like oracle.vae_ref.encode"""
    mean, logvar, std = R.posterior(tiled_encode_moments(P, cfg, x, T, S, f))
    return mean, logvar, (mean if noise is None else mean + std * noise)


def blend_closed_form64(rows, H, W, S, lim, ext):
    """rows[i][j]: [B, C, eh, ew] decoded tiles, tile (i, j) covering the output from (i * lim, j * lim). Returns float64
    (value, magnitude, in_band): the closed form over D[i][j], D[i-1][j], D[i][j-1], D[i-1][j-1] with exact-in-double weights, the
    same expression over |D| (= sum_k w_k |D_k|), and the [H, W] mask of the elements that are blended at all."""
    B, C = rows[0][0].shape[:2]
    val = torch.zeros(B, C, H, W, dtype=torch.float64)
    mag = torch.zeros_like(val)
    band = torch.zeros(H, W, dtype=torch.bool)
    rows64 = [[t.double() for t in row] for row in rows]

    def ext_of(k, N):
        return min(S, N - k * lim)

    for Y in range(H):
        i = Y // lim
        y = Y - i * lim
        ev = min(ext_of(i - 1, H), ext_of(i, H), ext) if i else 0
        iv = y < ev
        ry = ext_of(i - 1, H) - ev + y if iv else 0
        wy = y / ev if iv else 1.0
        for j in range(-(-W // lim)):
            x0, ew = j * lim, min(ext_of(j, W), lim)
            eh_ = min(ext_of(j - 1, W), ext_of(j, W), ext) if j else 0
            D = lambda a, b: rows64[a][b]  # noqa: E731
            cur = D(i, j)[:, :, y, :ew]
            wx = torch.ones(ew, dtype=torch.float64)
            wx[:eh_] = torch.arange(eh_, dtype=torch.float64) / max(eh_, 1)
            for k, absf in ((val, lambda t: t), (mag, torch.abs)):
                c = absf(cur)
                if iv:
                    tr = absf(D(i - 1, j)[:, :, ry, :ew])
                    top = tr.clone()
                if eh_:
                    cx0 = ext_of(j - 1, W) - eh_
                    bl = absf(D(i, j - 1)[:, :, y, cx0:cx0 + eh_])
                    if iv:
                        tl = absf(D(i - 1, j - 1)[:, :, ry, cx0:cx0 + eh_])
                        top[..., :eh_] = tl * (1 - wx[:eh_]) + tr[..., :eh_] * wx[:eh_]
                        left = tl * (1 - wy) + bl * wy
                    else:
                        left = bl
                v = top * (1 - wy) + c * wy if iv else c
                if eh_:
                    v = v.clone()
                    v[..., :eh_] = left * (1 - wx[:eh_]) + v[..., :eh_] * wx[:eh_]
                k[:, :, Y, x0:x0 + ew] = v
            band[Y, x0:x0 + ew] = iv
            band[Y, x0:x0 + eh_] = True
    return val, mag, band
