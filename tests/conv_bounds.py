"""Float64 references and elementwise error bounds for the convolution kernels: the implicit-GEMM 3 x 3 convolution
(mi355x_sd_conv3x3 -> csrc/gemm.hip, gemm_pipe.hip, gemm256.hip) and the three direct kernels of csrc/misc.hip. Plain Python + torch;
runs on whatever device the tensors live on.

The reference side is independent of the kernels: im2col() builds the [M, 9, Cin] operand with F.interpolate(nearest), F.pad and
F.unfold only -- none of the kernels' index arithmetic (output origin times stride plus tap minus padding, the upsample shift)
appears here. The bound for mi355x_sd_conv3x3 is tests/gemm_bounds.py's with K = 9 Cin on im2col(x).reshape(M, 9 Cin) and the weights
in logical [Cout][3][3][Cin] order (from_kb64() un-permutes MI355X_SD_CONV_KB64 weights on the host); see that file for rowbias, the
fp32 residual, the fp32 output and split-K. check() is gemm_bounds.check: worst |out - ref| / bound over every element, pass < 1.0.

Direct kernels (u32 = 2^-24; S = sum_k |a_k w_k| over the taps inside the image; a = the rounded operand the kernel documents):

  * conv_in3x3 (x NCHW fp32, w [9 Cin][Cout]): a = elem(fp32(x * in_scale)) -- one fp32 multiply, one rounding to the element type, as
    `(float)(bf16)(x * xs)` does -- then ONE sequential fp32 fma chain per output, started at the bias, over the 9 Cin taps (padding
    taps are skipped or contribute exact zeros). A chain of n fused multiply-adds rounds n times and each rounding acts on a partial
    sum of magnitude <= |bias| + S:   e = 9 Cin * u32 * (|bias| + S).   Stored as 16 bits (u_out as in gemm_bounds) or as fp32.
  * conv_out3x3 (x NHWC 16-bit, w [Cout][9][Cin], y NCHW fp32): a lane owns NI chunks of 8 elements (NI = ceil(9 Cin / 8 / 64),
    rounded up to the instantiated count), every chunk is four packed-pair dot products accumulating into one fp32 (two products
    and two additions per instruction: two roundings counted for each), then a 64-lane butterfly sum (6 additions), then the bias
    (1):   e = (8 NI + 7) * u32 * (|bias| + S).   fp32 out.
  * conv1x1_nchw (x NCHW fp32, w [Cout][Cin], y NCHW fp32): a = elem(fp32(x * in_scale)), a sequential fma chain of Cin terms
    started at the bias:   e = Cin * u32 * (|bias| + S).   fp32 out.
"""
import torch
import torch.nn.functional as F

from tests import gemm_bounds as GB

check = GB.check   # (the GEMM's conventions: an fp32 output is the epilogue value itself, rel-L2 unclamped)
U32 = GB.U32


def im2col(x, stride=1, up=False, pad_br=False):
    """x [B, H, W, Cin] (any strides, any float type; values taken exactly) -> (float64 [M, 9, Cin], Ho, Wo): row m = (b, oy, ox) of the
    convolution's output, tap = 3 ky + kx. Nearest-2x upsample first when `up`; zero padding 1 all round, or bottom / right only
    when `pad_br` (the stride-2 downsampler's)."""
    B, H, W, C = x.shape
    t = x.double().permute(0, 3, 1, 2)
    if up:
        t = F.interpolate(t, scale_factor=2, mode="nearest")
    t = F.pad(t, (0, 1, 0, 1) if pad_br else (1, 1, 1, 1))
    Ho, Wo = (t.shape[2] - 3) // stride + 1, (t.shape[3] - 3) // stride + 1   # (the standard convolution output size of the padded image)
    cols = F.unfold(t, kernel_size=3, stride=stride)   # [B, Cin * 9, Ho * Wo], channel-major
    assert cols.shape[2] == Ho * Wo, (cols.shape, Ho, Wo)
    return cols.view(B, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9, C), Ho, Wo


def to_kb64(w):
    """[Cout, 9 Cin] logical ([Cout][3][3][Cin]) -> the MI355X_SD_CONV_KB64 packing [Cout][Cin / 64][3][3][64]"""
    N, K = w.shape
    return w.view(N, 9, K // 9 // 64, 64).permute(0, 2, 1, 3).reshape(N, K).contiguous()


def from_kb64(w):
    """the MI355X_SD_CONV_KB64 packing -> logical [Cout, 9 Cin]"""
    N, K = w.shape
    return w.view(N, K // 9 // 64, 9, 64).permute(0, 2, 1, 3).reshape(N, K).contiguous()


def conv3x3_reference(x, w, *, stride=1, up=False, pad_br=False, bias=None, rowbias=None, residual=None, out_scale=1.0, silu=False):
    """(ref, e) of mi355x_sd_conv3x3: x [B, H, W, Cin] exactly as the kernel reads it, w LOGICAL [Cout, 9 Cin], bias [Cout], rowbias
    [B, Cout], residual [M, Cout] (16-bit or fp32)."""
    a, Ho, Wo = im2col(x, stride, up, pad_br)
    return GB.reference(a.reshape(a.shape[0], -1), w, bias=bias, rowbias=rowbias, rows_per_batch=Ho * Wo, residual=residual,
                        out_scale=out_scale, act="silu" if silu else None)


def _chain(a, wt, bias, roundings):
    """ref = a @ wt + bias and e = roundings * u32 * (|bias| + |a| @ |wt|); a [M, K] float64, wt [K, N]"""
    W = wt.double()
    b = bias.double() if bias is not None else torch.zeros(W.shape[1], dtype=torch.float64, device=W.device)
    return a @ W + b, roundings * U32 * (a.abs() @ W.abs() + b.abs())


def conv_in3x3_reference(x_nchw, w, bias, in_scale, elem):
    """x fp32 [B, Cin, H, W], w [9 Cin, Cout] (k = tap * Cin + ci), in_scale a one-element fp32 tensor or None -> (ref, e) [B H W, Cout]"""
    xs = x_nchw.float() * (in_scale.float() if in_scale is not None else 1.0)   # (one fp32 multiply)
    a, _, _ = im2col(xs.to(elem).permute(0, 2, 3, 1))
    return _chain(a.reshape(a.shape[0], -1), w, bias, 9 * x_nchw.shape[1])


_CONV_OUT_NI = (1, 2, 3, 4, 6, 9, 12)   # the instantiated chunks-per-lane counts (misc.hip launch_conv_out3x3)


def conv_out3x3_reference(x, w, bias):
    """x [B, H, W, Cin] 16-bit view, w [Cout, 9 Cin] -> (ref, e) NCHW [B, Cout, H, W]"""
    B, H, W, Cin = x.shape
    ni = min(n for n in _CONV_OUT_NI if n >= (9 * (Cin // 8) + 63) // 64)
    a, _, _ = im2col(x)
    ref, e = _chain(a.reshape(a.shape[0], -1), w.t(), bias, 8 * ni + 7)
    nchw = lambda t: t.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()
    return nchw(ref), nchw(e)


def conv1x1_nchw_reference(x_nchw, w, bias, in_scale, elem):
    """x fp32 [B, Cin, H, W], w [Cout, Cin], in_scale a Python float (rounded to fp32 by the C ABI) -> (ref, e) NCHW"""
    B, Cin, H, W = x_nchw.shape
    s = torch.tensor(in_scale, dtype=torch.float32, device=x_nchw.device)
    a = (x_nchw.float() * s).to(elem).double().permute(0, 2, 3, 1).reshape(-1, Cin)
    ref, e = _chain(a, w.t(), bias, Cin)
    nchw = lambda t: t.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()
    return nchw(ref), nchw(e)
