"""Elementwise float64 error bound for the GEMM kernels (csrc/gemm*.hip): every output element is held to a bound derived from the
kernel's arithmetic, against a float64 reference computed from the exact 16-bit operands. Plain Python + torch; runs on whatever
device the tensors live on.

Derivation. A kernel multiplies 16-bit operands exactly (a bf16 / fp16 product fits in fp32) and sums them in fp32: a 32-deep
v_mfma_f32_16x16x32 step adds 32 products to its accumulator, K / 32 such steps chain. With unit roundoff u32 = 2^-24 and at most
K / 32 + 32 roundings on any product's way into the sum (the chain plus the inside of one MFMA step), the accumulator satisfies

    |acc - sum_k a_k w_k| <= gamma_K * sum_k |a_k w_k|,      gamma_K = (K / 32 + 32) * 2^-24

and sum_k |a_k w_k| is one float64 |A| @ |W|^T. Weight-only fp8 (WS) runs on the widened matrix: acc = A . Q^T then * scale, so the
same bound holds with W = dequantize_fp8_rows(Q, scale) (the scale is positive).

Epilogue, in fp32, the order of gemm_epilogue.h epi4: z = ((acc + bias) * gate + R) * out_scale. Bias, gate and out_scale are
linear, so the accumulator error arrives at z multiplied by |gate * out_scale|. The epilogue's own fp32 roundings (bias add, gate
multiply, residual add, scale: at most EPI_OPS of them) add EPI_OPS * 2^-24 times the magnitudes they act on,
(|acc| + |bias|) |gate| + |R|, times |out_scale|. The residual R is a 16-bit tensor read exactly, so its only error is that add.

    e_z = |out_scale| * ( |gate| gamma_K S + EPI_OPS 2^-24 ((|acc| + |bias|) |gate| + |R|) )

Activations: out = f(z) with |f(z + e) - f(z)| <= L_f |e|, L_f the maximum slope of f over R (SiLU 1.0999 -> 1.10; erf-GELU 1.1289
and tanh-GELU 1.1295 -> 1.13), plus the device form's own approximation error as a stated constant:
  * SiLU and tanh-GELU are x * sigmoid(.) with v_exp_f32 / v_rcp_f32 (a few fp32 ulps): ACT_REL = 2^-20 relative to |z|;
  * erf-GELU (GEGLU's gate) is x * sigmoid(p(x)) with p a fitted quintic, 2.6e-5 absolute on Phi (common.h gelu_erf_f):
    GELU_ERF_ABS = 3e-5 times max(|g|, 1).
GEGLU pairs a value h and a gate g: out = h * gelu(g), so
    e_out = |gelu(g)| e_h + (|h| + e_h) (1.13 e_g + GELU_ERF_ABS max(|g|, 1)).

Finally the 16-bit store rounds once: |fl(y) - y| <= u |y| with u = 2^-8 for bf16 (8 significand bits) and 2^-11 for fp16. The
bound takes u_out = 2 u -- 2^-7 for bf16, 2^-10 for fp16 -- so that a correct kernel sits at or below half of it; the kernel's y
is itself off by e, hence

    |out - ref| <= u_out |ref| + (1 + u_out) e + 2^-24         (the last term: fp16's subnormal spacing)

Convolutions (tests/conv_bounds.py: K = 9 Cin on the im2col matrix) add three operands. rowbias [batches, N] is indexed like the
gate, m // rows_per_batch, and added with the bias: its magnitude joins the bias's in the epilogue term. The residual may be fp32
(r_f32): read exactly like the 16-bit one, its only error is the add. With bias, rowbias, residual and out_scale all present
gemm_epilogue.h epi4 rounds four times -- bias add, rowbias add (the batched form adds rowbias + fp32 residual first, then that sum:
still one rounding per operand), residual add, scale; a bias that starts the accumulators (bias_acc) saves one -- so EPI_OPS = 4 holds
and is not raised. An fp32 output (OUT_F32) is the epilogue value itself: u_out = 0 and the bound is e + 2^-24 |ref| (the reference
is compared in float64; 2^-24 |ref| is the fp32 representation of the value). Split-K needs no constant: a slice of kc K-tiles chains 2 kc MFMA steps, the reduce
kernel (splitk_reduce_kernel) adds the s slices in index order, 2 kc + s roundings on a product's way in all. plan_splitk slices a
launch of at most 160 tiles of 128 x 128 with nt = ceil(K / 64) >= 8 K-tiles into 2 <= s <= nt / 4 slices of kc = ceil(nt / s) <=
nt / s + 1 K-tiles (the last slice may be shorter): 2 kc + s <= 2 nt / s + 2 + s, which is convex in s and at both ends -- nt + 4 at
s = 2, 10 + nt / 4 at s = nt / 4 -- at most 2 nt for nt >= 8. The unsliced chain has 2 nt steps (a ragged last K-tile adds exact
zeros), so gamma_K covers every plan.

A bias that starts the accumulators (GemmArgs::bias_acc: the pipelined loops of gemm_pipe.hip and the small tile of gemm_small.hip
on 16-bit weights, no split-K, no LayerNorm fold) is no epilogue operand any more: it rides the whole chain, every partial sum is
bounded by |bias| + S, and the accumulator term becomes gamma_K (S + |bias|). Callers whose launch may take that form pass
bias_acc=True; the four-wave tile and the generic loop add the bias in the epilogue and leave it False.

In-kernel e4m3 weights (the W8 instantiations of the generic loop, routes +f8): the fragments are widened exactly, acc = A . Q^T, and
gemm_epilogue.h epi4 multiplies by the channel's scale FIRST (`v *= wsc`), then adds the bias: z = ((acc * scale + bias + rowbias) *
gate + R) * out_scale. Callers pass W = Q * scale (computed in float64 so that it is the exact product; the scale is positive), which
makes gamma_K S the scaled accumulator term. The scale multiply is one more fp32 rounding, on |acc * scale|. What Python reaches
(ops.linear_ex with w_scale) has scale, bias, gate and residual -- four roundings, out_scale is 1.0 and multiplies exactly, there is
no rowbias -- so EPI_OPS holds; `acc * scale + bias` contracted into one FMA under -ffp-contract=fast only saves one. Through the C
ABI all six operands can meet (scale, bias, rowbias, gate, residual, out_scale): such a caller passes epi_ops=6. The module
constant stays 4.

LayerNorm fold (gemm_epilogue_ln, routes +ln and the LN instantiations of the pipelined loops, the small tile, the phased kernel and
the split-K reduce kernel): rowstat [M, 2] = (rstd, nmr = -mean * rstd) and wsum [N], both fp32 and both taken exactly as the
kernel reads them (tests/norm_bounds.py bounds row_stats itself), give

    z = rstd[m] * acc + nmr[m] * wsum[n] + bias[n]

so the accumulator term arrives as |rstd| gamma_K S. The code is `v = rs[0] * acc + rs[1] * wsum; if (bias) v += bias`: a multiply,
then either a multiply and an add or -- contracted -- one FMA, then the bias add: at most four roundings (EPI_OPS), each on a partial
result bounded by |rstd * acc| + |nmr * wsum| + |bias|. The two products nearly cancel when the row mean is large against the row
deviation; the roundings do not know that, so the magnitudes are summed, not the terms:

    e_z = |rstd| gamma_K S + EPI_OPS 2^-24 (|rstd * acc| + |nmr * wsum| + |bias|)

dispatch_gemm refuses gate / rowbias / residual / fp8 scale next to the fold, and mi355x_sd_linear_ln has no out_scale; GEGLU and the
activations follow as above.

check() returns the worst |out - ref| / bound over the WHOLE output (the margin the logs show; a correct kernel stays below ~0.5, a
wrong sub-tile or a doubled bias lands far above 1) and the rel-L2 of the same comparison.
"""
import torch

from tests import bound_pieces as BP
from tests.bound_pieces import U32, U_OUT  # noqa: F401  (U_OUT: for the importers of this module)

EPI_OPS = 4
SLOPE = {"silu": 1.10, "gelu_tanh": 1.13, "gelu_erf": 1.13}
ACT_REL = 2.0 ** -20
GELU_ERF_ABS = 3e-5


def gamma(K: int) -> float:
    """fp32 accumulation error factor of a K-deep sum in chains of 16x16x32 MFMAs"""
    return (K / 32 + 32) * U32


def _act(name, z):
    if name == "silu":
        return z * torch.sigmoid(z)
    if name == "gelu_tanh":
        return torch.nn.functional.gelu(z, approximate="tanh")
    if name == "gelu_erf":
        return torch.nn.functional.gelu(z)
    raise ValueError(name)


def reference(a, w, *, bias=None, w_scale=None, out_scale=1.0, act=None, geglu=False, gate=None, rows_per_batch=0,
              residual=None, rowbias=None, rowstat=None, wsum=None, bias_acc=False, epi_ops=EPI_OPS):
    """float64 reference and elementwise accumulator-side error e (before the output rounding) of
    out = act(((a @ w^T) * w_scale + bias + rowbias[m // rows_per_batch]) * gate[m // rows_per_batch] + residual) * out_scale ...,
    or the GEGLU form. a [M, K], w [N, K] (for WS: the dequantized weights, w_scale None), bias [N], gate and rowbias
    [batches, N], residual [M, N] (16-bit, or fp32 for r_f32 launches): the logical operands exactly as the kernel reads them.
    rowstat [M, 2] fp32 (rstd, -mean * rstd) with wsum [N] fp32: the LayerNorm-folded form z = rstd * acc + nmr * wsum + bias.
    bias_acc: the bias starts the accumulators; epi_ops: the epilogue's fp32 roundings where a form has more than EPI_OPS (the
    module docstring derives both)."""
    M, K = a.shape
    A, W = a.double(), w.double()
    acc = A @ W.t()
    e = gamma(K) * (A.abs() @ W.abs().t())
    del A, W
    if w_scale is not None:   # (callers pass dequantized weights instead; kept for completeness)
        acc = acc * w_scale.double()
        e = e * w_scale.double().abs()
    b = bias.double() if bias is not None else torch.zeros(acc.shape[1], dtype=torch.float64, device=acc.device)
    if bias_acc:
        e = e + gamma(K) * b.abs()
    if rowstat is not None:
        rstd, nmr = rowstat.double()[:, :1], rowstat.double()[:, 1:]
        corr = nmr * wsum.double()
        acc, e = rstd * acc, rstd.abs() * e
        mag = acc.abs() + corr.abs() + b.abs()
        z = acc + corr + b
        del corr
    else:
        mag = acc.abs() + b.abs()
        z = acc + b
    del acc
    if rowbias is not None:
        rb = rowbias.double()[torch.arange(M, device=z.device) // rows_per_batch]
        z, mag = z + rb, mag + rb.abs()
        del rb
    if gate is not None:
        g = gate.double()[torch.arange(M, device=z.device) // rows_per_batch]
        z, e, mag = z * g, e * g.abs(), mag * g.abs()
        del g
    if residual is not None:
        r = residual.double()
        z, mag = z + r, mag + r.abs()
        del r
    e = abs(out_scale) * (e + epi_ops * U32 * mag)
    z = z * out_scale
    del mag
    if geglu:
        N = z.shape[1]
        zz, ee = z.reshape(M, N // 32, 2, 16), e.reshape(M, N // 32, 2, 16)
        h, g, eh, eg = zz[:, :, 0], zz[:, :, 1], ee[:, :, 0], ee[:, :, 1]
        gg = _act("gelu_erf", g)
        ref = (h * gg).reshape(M, N // 2)
        e = (gg.abs() * eh + (h.abs() + eh) * (SLOPE["gelu_erf"] * eg + GELU_ERF_ABS * g.abs().clamp_min(1.0))).reshape(M, N // 2)
        return ref, e
    if act is not None:
        e = SLOPE[act] * e + ACT_REL * z.abs()
        z = _act(act, z)
    return z, e


def check(out, ref, e):
    """(worst |out - ref| / bound over every element, rel-L2) of a 16-bit or fp32 output against reference() (non-finite -> inf).
    fp32: u_out = 0, the epilogue value stored as it is, so the bound is e + 2^-24 |ref|. rel-L2's denominator is not clamped."""
    return BP.check(out, ref, e, f32_rel=U32, rel_floor=0.0)


def bound_check(out, a, w, **kw):
    """reference() + check() in one call: (worst err / bound, rel-L2)"""
    ref, e = reference(a, w, **kw)
    return check(out, ref, e)
