"""Float64 references and the elementwise error bound of mi355x_sd_freeu (csrc/freeu.hip), shared by the host tests, the emulator and
the GPU child. No kernel output went into any number here.

REFERENCE. ``fourier_filter`` / ``apply_freeu`` are float64 ``torch.fft`` restatements of the reference's functions of the same names
(ppdiffusers/utils/paddle_utils.py:259-313): fftn over the last two axes, fftshift, the mask that is ``scale`` on
[crow - t, crow + t) x [ccol - t, ccol + t) and 1 elsewhere, ifftshift, ifftn, the real part. ``closed_form`` is what the kernel
evaluates: with threshold 1 the mask covers the shifted bins ky, kx in {-1, 0}, and for a real plane

    out = x + (s - 1) (<x> + sum over phi in {ty, tx, ty + tx} of <x cos phi> cos phi + <x sin phi> sin phi),
    ty = 2 pi y / H, tx = 2 pi x / W, <.> the mean over the plane.

The +-1 components are scaled by HALF of (s - 1) (the box holds one bin of each conjugate pair) -- except on an axis of length 2, whose
bin -1 is its own conjugate --, and the ty - tx component is not touched. ``closed_form(mutant=...)`` states the three ways of getting
that wrong; tests/test_freeu_host.py holds each above the bound.

LAUNCH. ``cols`` / ``rows_per_split`` / ``launch`` restate the launcher's heuristics (freeu_cols, freeu_rows_per_split,
freeu_launch): 16-byte column groups aligned to the row start, at most 64 groups per grid column, 256 // gw row slots per block, and
the plane's rows split over blockIdx.y until 512 blocks exist (at most 32 splits, never more than leave every row slot a row).
``SPLIT_SHAPE`` is the smallest plane of the test matrix the split engages on.

BOUND. Every stored element is held (rowmap_bounds.check) to |out - ref| <= u |ref| + (1 + u) e + 2^-24 for a 16-bit store and
2 u32 |ref| + e for an fp32 store, ref the float64 value from the exact operands. e, for a skip element, from the kernel's arithmetic:
  * a trigonometric value: sincospif at <= 2 ulp of a value <= 1 (SINCOS_ABS = 4 u32, rowmap_bounds), its argument 2 r / n, |.| <= 1,
    one rounding: pi u32 on the angle. TRIG = (4 + pi) u32 absolute. cos / sin (ty + tx) are sums of two products of two such
    values: 2 TRIG + 3 u32 <= 3 TRIG.
  * a sum S_q: per pixel a product with a trig value and an addition; the additions form a chain of
    L = W (a row) + ceil(rows per split / ty) (a thread's rows) + ty (the block's slots) + splits (the apply pass) links, each
    product and the row's combination a few more: gamma(L + 8) A, A = sum |x| over the plane, plus the trig error 3 TRIG A.
  * the correction (s - 1) / HW * sum_q S_q t_q: seven terms, each |dS_q| + |S_q| 3 TRIG, |S_q| <= A, and at most 8 more roundings
    (k, E / F / G, the three fused multiply-adds): 8 u32 A each.
  * x + correction: one rounding of |x| + |correction|, taken twice.
  e = |s - 1| <|x|> 7 (gamma(L + 8) + 6 TRIG + 8 u32) + 2 u32 (|x| + 7 |s - 1| <|x|>).
A backbone element is x * b: e = u32 |x b|. Untouched columns and the row padding are compared bit for bit."""
import math

import torch

from tests.gemm_bounds import U32
from tests.norm_bounds import fp32, gamma
from tests.rowmap_bounds import SINCOS_ABS, check  # noqa: F401  (check: what the callers hold the output to)

TRIG = SINCOS_ABS + math.pi * U32
THREADS, LANES, TARGET_BLOCKS, MAX_SPLIT = 256, 64, 512, 32

SIZES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 4), (5, 7), (8, 8), (16, 12), (32, 32), (6, 10)]   # (the last: H != W, no power of two)
FREEU = dict(s1=0.9, s2=0.2, b1=1.3, b2=1.4)   # the whole-U-Net setting of the tests


# ---- references -------------------------------------------------------------------------------------------------------------------
def fourier_filter(x, threshold, scale):
    """paddle_utils.py:259-287 in float64; x [..., H, W]"""
    x = x.double()
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real


def apply_freeu(resolution_idx, hidden, res, s1, s2, b1, b2):
    """paddle_utils.py:289-313 in float64 on NCHW tensors -> (hidden, res)"""
    hidden, res = hidden.double().clone(), res.double()
    if resolution_idx in (0, 1):
        half = hidden.shape[1] // 2
        hidden[:, :half] = hidden[:, :half] * (b1, b2)[resolution_idx]
        res = fourier_filter(res, 1, (s1, s2)[resolution_idx])
    return hidden, res


def angles(H, W):
    ty = (2 * math.pi / H) * torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    tx = (2 * math.pi / W) * torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    return ty, tx


def closed_form(x, s, mutant=None):
    """the rank-7 correction, float64, x [..., H, W]. mutant: "drop_sum" (no ty + tx term), "scale_diff" (ty - tx scaled too),
    "full_pm1" (the whole (s - 1) on the ty component instead of half)"""
    x = x.double()
    H, W = x.shape[-2:]
    ty, tx = angles(H, W)
    mean = lambda t: t.mean(dim=(-2, -1), keepdim=True)  # noqa: E731
    phis = [(ty, 1.0), (tx, 1.0), (ty + tx, 1.0)]
    if mutant == "drop_sum":
        phis = phis[:2]
    elif mutant == "scale_diff":
        phis.append((ty - tx, 1.0))
    elif mutant == "full_pm1":
        phis[0] = (ty, 2.0)
    elif mutant is not None:
        raise ValueError(mutant)
    corr = mean(x)
    for phi, w in phis:
        corr = corr + w * (mean(x * phi.cos()) * phi.cos() + mean(x * phi.sin()) * phi.sin())
    return x + (s - 1.0) * corr


# ---- launch heuristics (csrc/freeu.hip) -------------------------------------------------------------------------------------------
def cols(c0, c1, vec):
    """(g0, ng, nc, gw, ty) of the column span [c0, c1)"""
    if c1 <= c0:
        return (0, 0, 0, 1, THREADS)
    g0 = c0 // vec
    ng = (c1 + vec - 1) // vec - g0
    nc = (ng + LANES - 1) // LANES
    gw = (ng + nc - 1) // nc
    return (g0, ng, nc, gw, THREADS // gw)


def rows_per_split(B, H, nc, ty):
    blocks = B * max(nc, 1)
    want = min((TARGET_BLOCKS + blocks - 1) // blocks, (H + ty - 1) // ty, MAX_SPLIT)
    want = max(want, 1)
    return (H + want - 1) // want


def launch(B, H, W, Cx, Cs, f32):
    """dict(vec, gw, ty, rps, splits, chain) of the statistics launch; chain: the links of the longest addition chain behind a sum"""
    vec = 4 if f32 else 8
    _, _, nc, gw, ty = cols(Cx, Cx + Cs, vec)
    rps = rows_per_split(B, H, nc, ty)
    splits = (H + rps - 1) // rps
    return dict(vec=vec, gw=gw, ty=ty, rps=rps, splits=splits, chain=W + (rps + ty - 1) // ty + ty + splits)


def workspace_floats(B, H, W, Cs):
    if B < 1 or H < 2 or W < 2 or Cs < 1:
        return 0
    return B * min(H, MAX_SPLIT) * 7 * (Cs + 16)


# the smallest plane on which the rows ARE split: Cs = 64 16-bit channels are 8 column groups -> 32 row slots per block, so a plane
# of more than 32 rows takes two splits at B = 2 (2 blocks << 512); W = 4 keeps it small
SPLIT_SHAPE = (40, 4)
assert launch(2, *SPLIT_SHAPE, 0, 64, False)["splits"] == 2 and launch(2, 16, 12, 0, 64, False)["splits"] == 1

# the smallest kind of channel counts at which BOTH column spans -- the scaled backbone half [0, Cx // 2) and the skip span
# [Cx, Cx + Cs) -- are more than 64 column groups, for both element sizes: more than one grid column each (the blockIdx.x * gw + gl
# indexing, the blockIdx.x - A.nc offset of the apply pass, the workspace addressed across grid columns), and the groups do not divide
# evenly, so the last grid column has lanes past the span (the g >= ng tail). Cx is odd: both ends of the skip span straddle a group.
WIDE_CHANNELS = (1041, 531)   # (Cx, Cs)
WIDE_SHAPES = [(2, 2), (3, 5)]
for _vec in (8, 4):
    for _span in ((0, WIDE_CHANNELS[0] // 2), (WIDE_CHANNELS[0], sum(WIDE_CHANNELS))):
        _g0, _ng, _nc, _gw, _ty = cols(*_span, _vec)
        assert _nc > 1 and _nc * _gw > _ng, (_vec, _span, _ng, _nc, _gw)


# ---- the call as the kernel sees it -----------------------------------------------------------------------------------------------
def expected(rows, B, H, W, Cx, Cs, b, s, f32):
    """rows: the [B*H*W, ld] buffer before the call (any float dtype; the exact operands). -> (ref, e) float64 [B*H*W, Cx + Cs]:
    the reference of the written columns and the bound's e; columns [Cx // 2, Cx) keep ref = input, e = 0."""
    b, s = fp32(b), fp32(s)
    x = rows[:, :Cx + Cs].double()
    ref, e = x.clone(), torch.zeros_like(x)
    half = Cx // 2
    ref[:, :half] = x[:, :half] * b
    e[:, :half] = U32 * ref[:, :half].abs()
    planes = x[:, Cx:].reshape(B, H, W, Cs).permute(0, 3, 1, 2)
    filt = fourier_filter(planes, 1, s)
    ref[:, Cx:] = filt.permute(0, 2, 3, 1).reshape(B * H * W, Cs)
    L = launch(B, H, W, Cx, Cs, f32)["chain"]
    mabs = planes.abs().mean(dim=(-2, -1), keepdim=True).expand_as(planes)
    ep = abs(s - 1.0) * mabs * 7 * (gamma(L + 8) + 6 * TRIG + 8 * U32) + 2 * U32 * (planes.abs() + 7 * abs(s - 1.0) * mabs)
    e[:, Cx:] = ep.permute(0, 2, 3, 1).reshape(B * H * W, Cs)
    return ref, e


def planes_input(kind, B, H, W, C, seed=0):
    """[B, C, H, W] float64 test planes: "normal", "dc" (offset 1e3 x the spread), "cos_ty" | "cos_tx" | "cos_sum" | "cos_diff" (pure
    components, a different amplitude per plane)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    if kind == "dc":
        return 1e3 + torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    ty, tx = angles(H, W)
    phi = dict(cos_ty=ty, cos_tx=tx, cos_sum=ty + tx, cos_diff=ty - tx)[kind]
    amp = 0.5 + torch.rand(B, C, 1, 1, generator=g, dtype=torch.float64)
    return amp * phi.cos()


KINDS = ("normal", "dc", "cos_ty", "cos_tx", "cos_sum", "cos_diff")


# ---- whole U-Net: the oracle with FreeU ---------------------------------------------------------------------------------------------
def patch_oracle(monkeypatch, cfg, s1, s2, b1, b2):
    """wraps oracle.unet_ref.resnet_block: the concatenated input of up_blocks.{0,1}.resnets.* gets apply_freeu, split at the Cx the
    structure walk gives (the ('cat', skip_c) row in front of each up resnet)"""
    from oracle import unet_ref as U
    from paddlemix_amd.unet import _structure, normalize_config
    S = _structure(normalize_config(cfg))
    skip_c = {S[i + 1][1]: d[1] for i, d in enumerate(S) if d[0] == "cat"}
    orig = U.resnet_block

    def resnet_block(P, name, x, *a, **k):
        if name.startswith(("up_blocks.0.", "up_blocks.1.")):
            cx = x.shape[1] - skip_c[name]
            hid, res = apply_freeu(int(name.split(".")[1]), x[:, :cx], x[:, cx:], s1, s2, b1, b2)
            x = torch.cat([hid, res], dim=1).to(x.dtype)
        return orig(P, name, x, *a, **k)

    monkeypatch.setattr(U, "resnet_block", resnet_block)
