"""Inputs for the convolution kernels on which a wrong gather cannot hide (tests/conv_child.py on the GPU, tests/test_conv_bounds.py on
the CPU). Every value is exact in bf16 and in fp16. Three kinds, each usable with every geometry and both K orders:

  coded   x[b, y, x, c] is a non-zero integer of magnitude <= 126 that differs between any two pixels within two steps in y and x,
          between channels c and c + 1, c + 8, c + 64, and between batch items; output channel n has a single 1.0 at
          k(n) = (p n + s) % (9 Cin), p coprime to 9 Cin and small enough that every tap and every 64-wide K-tile is selected. Then
          out[m, n] is ONE input element or the padding zero: compared with torch.equal, not with a bound. No bias.
  mask    x = 1 everywhere; output channel 2 j carries 2^tap for taps 0..4 and channel 2 j + 1 carries 2^(tap - 5) for taps 5..8, in
          one input channel c_j that walks the 8-channel blocks. Every output is an integer <= 31 that names the taps that fell inside
          the image: exact equality again. Pins both padding rules, the stride and the upsample at every output pixel.
  random  normal data with bias, rowbias (a column slice of a wider fp32 table), residual (16-bit or fp32), out_scale, SiLU, fp32
          output: held to the float64 bound of tests/conv_bounds.py.

Buffers: x is a channel slice of a wider NHWC allocation (pixel stride Cin + 24, first channel 8), the gap channels and one image's
worth of elements before and after the tensor are NaN. The output is a column slice of a canary-filled buffer with canary rows above
and below (tests/kernel_pieces.py Guarded.block); its counts() give the disturbed canary elements.
"""
import math
from collections import namedtuple

import torch

from tests import conv_bounds as CB
from tests import kernel_pieces as KP

# geometry name -> (stride, upsample, pad_br): every combination mi355x_sd_conv3x3 accepts (pad_br is the stride-2 downsampler's)
GEOMS = {"s1": (1, False, False), "s1up": (1, True, False), "s2": (2, False, False), "s2up": (2, True, False), "s2br": (2, False, True)}
Case = namedtuple("Case", "kind B H W Cin Cout geom kb64 epi")
X_GAP, X_OFF = 24, 8        # spare channels per pixel of the wider NHWC allocation, first channel of the slice
C_GAP, C_OFF, C_ROWS = 16, 8, 64   # spare columns / first column / canary rows above and below the output


def _cases():
    c = {}
    # selector grid: every geometry x both K orders x both selector kinds, B >= 2, odd H != W, Cout ragged against 128/160/256/320
    for g in GEOMS:
        for kb in (False, True):
            o = "kb64" if kb else "plain"
            cin = 128 if kb else 64   # (at Cin = 64 the two K orders are the same order: one channel block)
            c[f"coded {g} {o}"] = Case("coded", 3, 13, 9, cin, 328, g, kb, ())
            c[f"mask {g} {o}"] = Case("mask", 2, 5, 7, cin, 136, g, kb, ())
    # K edges: K = 72 and 360 are no multiples of 64 (a K tail; at Cin = 40 a K-tile straddles taps) -- plain K order only
    for cin in (8, 40):
        for g in ("s1", "s2up", "s2br"):
            c[f"coded {g} cin{cin}"] = Case("coded", 2, 7, 5, cin, 72, g, False, ())
        c[f"mask s2 cin{cin}"] = Case("mask", 2, 5, 7, cin, 40, "s2", False, ())
    # deep K, Cout a multiple of the tile widths and ragged
    c["coded s1 cin320 plain"] = Case("coded", 2, 7, 5, 320, 320, "s1", False, ())
    c["coded s2 cin320 kb64"] = Case("coded", 2, 7, 5, 320, 644, "s2", True, ())
    c["coded s1up cin640 kb64"] = Case("coded", 2, 3, 5, 640, 644, "s1up", True, ())
    c["mask s2br cin640 plain"] = Case("mask", 2, 5, 7, 640, 320, "s2br", False, ())
    # one pixel and 2 x 3 pixels with every geometry the entry point accepts, both K orders (Cin = 128 where they differ) and both
    # selector kinds (a 1 x 1 image has no pad_br output: tests/test_gpu_convs.py), then the epilogue operands at these sizes
    for g in GEOMS:
        for kb in (False, True):
            o, cin = ("kb64", 128) if kb else ("plain", 64)
            for kind in ("coded", "mask"):
                if g != "s2br":
                    c[f"{kind} 1x1 {g} {o}"] = Case(kind, 2, 1, 1, cin, 72, g, kb, ())
                c[f"{kind} 2x3 {g} {o}"] = Case(kind, 2, 2, 3, cin, 72, g, kb, ())
    c["random 2x3 s1 all16 silu"] = Case("random", 2, 2, 3, 64, 72, "s1", False, ("bias", "rowbias", "r16", "scale", "silu"))
    c["random 2x3 s2br kb64 rowbias+r32 f32 out"] = Case("random", 2, 2, 3, 128, 72, "s2br", True, ("rowbias", "r32", "f32"))
    c["random 2x3 s2up kb64 bias"] = Case("random", 2, 2, 3, 128, 72, "s2up", True, ("bias",))
    c["random 1x1 s1up kb64 silu scale r32"] = Case("random", 2, 1, 1, 128, 72, "s1up", True, ("bias", "r32", "scale", "silu"))
    c["random 1x1 s2 all16"] = Case("random", 3, 1, 1, 64, 72, "s2", False, ("bias", "rowbias", "r16", "scale"))
    # more 256-row tiles than one round of the chip (256 CUs): 259 row tiles
    c["coded big s1 plain"] = Case("coded", 2, 181, 183, 64, 72, "s1", False, ())
    c["coded big s2br kb64"] = Case("coded", 2, 363, 367, 64, 72, "s2br", True, ())
    # split-K: 60 tiles of 128 x 128, 90 K-tiles in 7 slices of 13 with an uneven last slice of 12
    c["random deep plain"] = Case("random", 2, 23, 27, 640, 644, "s1", False, ("bias", "rowbias", "r16", "scale"))
    c["random deep kb64"] = Case("random", 2, 23, 27, 640, 644, "s1", True, ("bias",))
    # random data, every epilogue operand the entry point accepts
    c["random s1 bias"] = Case("random", 3, 13, 9, 64, 328, "s1", False, ("bias",))
    c["random s2 all16"] = Case("random", 3, 13, 9, 64, 328, "s2", True, ("bias", "rowbias", "r16", "scale"))
    c["random s1up rowbias+r32"] = Case("random", 3, 13, 9, 64, 328, "s1up", False, ("rowbias", "r32"))
    c["random s2br silu"] = Case("random", 3, 13, 9, 64, 328, "s2br", True, ("bias", "silu"))
    c["random s1 silu after scale"] = Case("random", 3, 13, 9, 128, 328, "s1", True, ("bias", "rowbias", "scale", "silu"))   # (scale first, then SiLU)
    c["random s2up f32 out"] = Case("random", 3, 13, 9, 64, 328, "s2up", False, ("bias", "r32", "scale", "f32"))
    c["random s2 cin40"] = Case("random", 3, 13, 9, 40, 328, "s2", False, ("bias", "r16"))
    c["random s1up cin320 kb64"] = Case("random", 2, 9, 11, 320, 320, "s1up", True, ("bias", "rowbias"))
    # SDXL shapes in the production K order: the UNet's 320 -> 320 resnet conv at 128 x 128 (time-embedding rowbias), the VAE decoder's
    # 512 -> 512 conv at 128 x 128 (256 tiles of 256 x 256: the picker's phased kernel)
    c["random sdxl unet 320 kb64"] = Case("random", 2, 128, 128, 320, 320, "s1", True, ("bias", "rowbias"))
    c["random sdxl vae 512 kb64"] = Case("random", 2, 128, 128, 512, 512, "s1", True, ("bias",))
    return c


CASES = _cases()


def out_hw(case):
    """(Ho, Wo) from torch's own convolution output size on a one-channel image of the case's geometry"""
    s, up, br = GEOMS[case.geom]
    return CB.im2col(torch.zeros(1, case.H, case.W, 1), s, up, br)[1:]


def exact16(t):
    """fp32 values rounded to bf16 and, below fp16's normal range, to zero: exact in both 16-bit types"""
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def coded_x(B, H, W, C, device):
    b, y, x, c = torch.meshgrid(torch.arange(B, device=device), torch.arange(H, device=device), torch.arange(W, device=device),
                                torch.arange(C, device=device), indexing="ij")
    v = (101 * b + 37 * y + 11 * x + 3 * c + 5 * (c // 8) + 13 * (c // 64)) % 251
    return (v - 125 + (v >= 125).long()).float()


def selector_k(Cout, K, seed):
    """k(n) = (p n + s) % K with p coprime to K; asserts that every tap and every 64-wide K-tile is selected"""
    p = max(5, -(-K // Cout))
    while math.gcd(p, K) != 1:
        p += 1
    k = (p * torch.arange(Cout) + seed % K) % K
    cin = K // 9
    assert set((k // cin).tolist()) == set(range(9)), "a tap is not selected"
    assert set((k // 64).tolist()) == set(range(-(-K // 64))), "a K-tile is not selected"
    return k


def mask_w(Cout, Cin):
    w = torch.zeros(Cout, 9, Cin)
    for j in range(Cout // 2):
        cj = (8 * j + j % 8) % Cin
        for tap in range(9):
            w[2 * j + (tap >= 5), tap, cj] = 2.0 ** (tap if tap < 5 else tap - 5)
    return w.reshape(Cout, 9 * Cin)


def nan_embedded(x):
    """x [B, H, W, C] values -> (view of the same shape inside a NaN-filled wider allocation, the flat allocation, first element):
    pixel stride C + X_GAP, first channel X_OFF, one image's worth of NaN before and after the tensor"""
    B, H, W, C = x.shape
    ldx = C + X_GAP
    img = H * W * ldx
    view, full = KP.nan_embed(x, (img, W * ldx, ldx, 1), img + X_OFF, (B + 2) * img)
    return view, full, img + X_OFF


def alloc_out(M, N, dtype, device):
    """the [M, N] output as a column slice of a canary buffer with C_ROWS canary rows above and below (KP.Guarded: .view, and
    .counts()[1] the number of canary elements that no longer hold the canary)"""
    return KP.Guarded.block(M, N, 32 if dtype == torch.float32 else 16, above=C_ROWS, below=C_ROWS, left=C_OFF, right=C_GAP - C_OFF,
                            dt=dtype, device=device)


def build(name, case, elem, device):
    """operands of one case on `device`: dict(x view, x_full, x_first, w (logical [Cout, 9 Cin]), w_dev (the packing the kernel takes), bias,
    rowbias, residual, out_scale, silu, out_f32, Ho, Wo, M)"""
    B, H, W, Cin, Cout = case.B, case.H, case.W, case.Cin, case.Cout
    K = 9 * Cin
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(case)
    M = B * Ho * Wo
    d = dict(Ho=Ho, Wo=Wo, M=M, bias=None, rowbias=None, residual=None, out_scale=1.0, silu=False, out_f32=False, sel=None)
    if case.kind == "coded":
        x = coded_x(B, H, W, Cin, device)
        d["sel"] = selector_k(Cout, K, seed).to(device)
        w = torch.zeros(Cout, K)
        w[torch.arange(Cout), d["sel"].cpu()] = 1.0
    elif case.kind == "mask":
        x = torch.ones(B, H, W, Cin, device=device)
        w = mask_w(Cout, Cin)
    else:
        x = exact16(torch.randn(B, H, W, Cin, generator=g)).to(device)
        w = exact16(torch.randn(Cout, K, generator=g) / math.sqrt(K))
        if "bias" in case.epi:
            d["bias"] = torch.randn(Cout, generator=g).to(device)
        if "rowbias" in case.epi:   # a column slice of a wider fp32 table (the UNet's time-embedding projections of all resnets)
            d["rowbias"] = torch.randn(B, Cout + 24, generator=g).to(device)[:, 8:8 + Cout]
        if "r16" in case.epi:
            d["residual"] = exact16(torch.randn(M, Cout, generator=g)).to(device).to(elem)
        if "r32" in case.epi:
            d["residual"] = torch.randn(M, Cout, generator=g).to(device)
        d["out_scale"] = 0.7 if "scale" in case.epi else 1.0
        d["silu"], d["out_f32"] = "silu" in case.epi, "f32" in case.epi
    d["x"], d["x_full"], d["x_first"] = nan_embedded(x.to(elem))
    d["w"] = w.to(device).to(elem)
    d["w_dev"] = CB.to_kb64(d["w"]) if case.kb64 else d["w"]
    return d


def expected(case, d):
    """(ref float64 [M, Cout], e or None): e is None for the selector kinds, whose outputs are exact"""
    s, up, br = GEOMS[case.geom]
    if case.kind == "coded":
        a, _, _ = CB.im2col(d["x"], s, up, br)
        return a.reshape(a.shape[0], -1)[:, d["sel"]], None
    if case.kind == "mask":
        a, _, _ = CB.im2col(d["x"], s, up, br)
        return a.reshape(a.shape[0], -1) @ d["w"].double().t(), None
    return CB.conv3x3_reference(d["x"], d["w"], stride=s, up=up, pad_br=br, bias=d["bias"], rowbias=d["rowbias"],
                                residual=d["residual"], out_scale=d["out_scale"], silu=d["silu"])


def judge(case, d, out):
    """-> dict(ratio, rel, mismatch): selectors by exact equality (mismatch = number of unequal elements; ratio 0 or inf), random data by
    the bound"""
    ref, e = expected(case, d)
    if e is None:
        bad = int((out.double() != ref).sum().item())   # (NaN != x: counted)
        return dict(ratio=0.0 if bad == 0 else float("inf"), rel=0.0, mismatch=bad)
    ratio, rel = CB.check(out, ref, e)
    return dict(ratio=ratio, rel=rel, mismatch=None)
