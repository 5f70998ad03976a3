"""Exact bits and an elementwise float64 bound for the W8A8 GEMM: the F8 instantiation of gemm256_kernel (csrc/gemm256.hip),
gemm_epilogue_f8 (csrc/gemm_epilogue.h), the entries mi355x_sd_linear_f8 / mi355x_sd_linear_f8_q. Plain Python + torch; runs on
whatever device the tensors live on. What the 16-bit families share with this one -- the activation constants, the output rounding,
check() -- comes from tests/gemm_bounds.py; only what W8A8 needs is added here.

Class 1, exact bits. The operands are small integers in e4m3: one matrix dense in {-8 .. 8}, the other with at most 16 nonzeros of
+-1, +-2 per row, at K positions that differ row by row and visit every 16-byte chunk position of the 128-byte K-tile over the
matrix. Every product, every partial sum (|acc| <= 256) and -- with power-of-two scales, or integer bias / residual and a gate out
of {+-1, +-2, 0.5} on operands shrunk so that the result keeps at most 8 significant bits -- every epilogue value is exactly
representable in fp32 and in both 16-bit types. The expected bits are therefore ref.to(ed) with no model of the instruction at all,
and one misread element of either operand moves some output by at least 1. Two mirror cases (A sparse / W dense, A dense / W sparse)
give both operands both roles. exact_reference() asserts the precondition (ref.to(ed).double() == ref) on the reference alone.

Class 2, float64 bound. A = qa * sa and W = qw * sw are exact float64 products of the e4m3 values and their fp32 scales.
  * e4m3 x e4m3 products are exact in fp32 (4 + 4 significand bits, exponents far inside the range).
  * One v_mfma_scale_f32_16x16x128_f8f6f4 adds 128 products to its accumulator, K / 128 such steps chain. With u32 = 2^-24 and at
    most K / 128 + STEP roundings on any product's way into the sum (the chain, plus STEP units of 2^-24 inside one step):

        |acc - sum_k a_k w_k| <= gamma8(K) * sum_k |a_k w_k|,      gamma8(K) = (K / 128 + STEP) * 2^-24

    STEP was derived as 128 (a sequential fp32 adder is the worst a 128-term sum can do); nobody had measured how this instruction
    sums its 128 products. A kernel that passes class 1 in every case exceeded 1.0 with it -- a finding about the instruction, not
    about the kernel -- so STEP was raised ONCE to 256 (a truncating adder: 2^-23 per add), and goes no further. Worst err / bound on
    the MI355X before -> after, all at one K-tile (K = 128, where the step term is all of gamma8): fp16 build "d 231x648x128 gate"
    1.077 -> 0.646, "nobias" 0.975 -> 0.508, "bias" / "c-remap" 0.935 -> 0.531; bf16 build "gate" 0.839 -> 0.496, "nobias" 0.752 ->
    0.494. K = 256: fp16 0.728 -> 0.464; K = 6144: 0.48 -> 0.48 (the chain term and the store dominate).
    What the instruction does, measured with 256 - 256 + 64 * 2^-g (two products of 16 x 16 that cancel, 64 small ones, all exact):
    for g <= 5 every small product counts; from g = 6 on exactly those small products are lost that share an aligned group of 8
    consecutive k with a large one (6, 7 or 14 of the 64, by where the large ones sit), whatever the smaller g. So the 8 products of
    a group are aligned to the group's largest and cut about 13 bits below it, before the groups are added: the error of one step is
    bounded by ~7 * 2^-13 of each group's largest product, not by 2^-24 per operation. On dense operands, whose products of a group
    lie within a few bits of each other, that is what the ratios above show; on operands with one product > 2^13 times its group
    neighbours the bound of this module does not hold, and no test here builds such operands (class 1's small integers stay within
    2^7 of each other and are summed exactly).
  * Epilogue, fp32, the order of gemm_epilogue_f8: v = acc * as[m] * ws[n] (two roundings), + bias, * gate, + R: EPI_OPS8 = 5
    roundings, each on a partial result bounded by (|acc as ws| + |bias|) |gate| + |R|; `v + bias` contracted into an FMA only saves
    one. The accumulator error arrives multiplied by |as ws gate|:

        e_z = |gate| gamma8 (|A| @ |W|^T) + EPI_OPS8 2^-24 ((|A @ W^T| + |bias|) |gate| + |R|)

  * tanh-GELU: SLOPE and ACT_REL of tests/gemm_bounds.py; the 16-bit store: U_OUT and check() of tests/gemm_bounds.py.

e4m3 output (mi355x_sd_linear_f8_q). Row scale: the code computes bound = 1.1f * (a_l2[m] * w_norm_max + bias_abs_max) and stores
max(bound, 1e-12) * (1 / 448): one contraction (or two roundings), fmaxf, a rounded constant and a multiply, so

    |c_scale[m] - s64| <= 4 * 2^-24 * s64,      s64 = float64(float32(1.1)) * (a_l2 * w_norm_max + bias_abs_max) / 448.

Bytes: with y the float64 reference after GELU, e its bound, and s the device's OWN c_scale[m], the accepted codes are those between
e4m3((y - e') / s) and e4m3((y + e') / s), both ends included, in e4m3 order, e' = e + 8 * 2^-24 |y| (448 / bound, the multiply and
the division's ulps). No byte may be NaN. An interval that holds more than one code decides nothing between them, so at most
MULTI_CAP = 5 % of the elements may have one -- a condition on the committed inputs, asserted on the CPU from the reference alone
(estimated at ~1.6 % for the dense cases with STEP = 128; the shares measured with STEP = 256 are below. The inputs were
shaped to meet it: dense_operands' large W row, exact_q_operands' row factor).

Measured on the MI355X (the case matrix of tests/gemm_f8_child.py, STEP = 256), the same in both builds unless stated:
    class 1     0 differing bits in all 82 cases of either build; the same operands through the e4m3 output: 0 bytes outside, 0 NaN,
                at most 5.0 % multi-code intervals
    class 2     worst err / bound bf16 0.496 ("d 231x648x128 gate+gelu"), fp16 0.646 ("d 231x648x128 gate"); rel-L2 at most 1.75e-3
                (bf16) and 2.27e-4 (fp16)
    e4m3 output 0 bytes outside their interval, 0 NaN; row scale at most 0.748 of its allowance; multi-code intervals 0.5 % .. 1.3 %
                without GELU, 3.3 % .. 4.4 % with it
    everywhere  unwritten 0, overwritten 0, wrapper_off 0; all ten refusals return status 2 and write nothing

emulate() is a torch fp32 restatement of the kernel (128-deep fp32 steps chained, the epilogue in the code's order, one rounding to
16 bits, the e4m3 store) with the planted mistakes of tests/test_gemm_f8_bounds.py.

"""
import math

import torch

from tests import bound_pieces as BP
from tests import gemm_bounds as GB
from tests.kernel_pieces import F8_NAN  # noqa: F401  (NaN in e4m3fn: the filler of every gap of A and W, the canary of the e4m3 output)

U32 = GB.U32
STEP = 256          # roundings inside one 16x16x128 step, in units of 2^-24 (raised once from the derived 128, see above)
EPI_OPS8 = 5        # as, ws, bias, gate, residual
MULTI_CAP = 0.05    # share of e4m3 outputs whose interval may hold more than one code
F8 = torch.float8_e4m3fn
KT = 128            # elements per K-tile (128 bytes), 16-byte chunks of 16 elements


def gamma8(K: int) -> float:
    """fp32 accumulation error factor of a K-deep sum in chains of 16x16x128 fp8 MFMAs"""
    return (K / KT + STEP) * U32


# ---- e4m3 ------------------------------------------------------------------------------------------------------------------------
def from_bytes(q):
    """uint8 e4m3fn bytes -> float64 values"""
    return q.view(F8).double()


def to_bytes(v):
    """values exactly representable in e4m3 (|v| <= 448) -> uint8 bytes"""
    q = v.float().to(F8)
    assert torch.equal(q.double(), v.double()), "not an e4m3 value"
    return q.view(torch.uint8)


def e4m3_round(x, toward_zero=False):
    """float64 -> the e4m3fn value (float64) nearest to it, ties to even, saturating at +-448 (what v_cvt_pk_fp8_f32 does with finite
    inputs); done in float64, not through fp32, so that an interval end is rounded once. toward_zero: a planted FAULT."""
    a = x.abs().clamp(max=448.0)
    _, ex = torch.frexp(a)                              # a = m * 2^ex, 0.5 <= m < 1
    ex = (ex - 1).clamp(min=-6)                         # floor(log2 a); the subnormals share the quantum of 2^-6
    quant = ((ex.long() - 3 + 1023) << 52).view(torch.float64)   # 2^(ex - 3), 3 mantissa bits; built from its bits: exact on any device
    r = a / quant
    r = torch.floor(r) if toward_zero else torch.round(r)
    return torch.copysign(r * quant, x)


def quantize_rows(x):
    """per-row e4m3 quantisation as the model does: (uint8 [rows, C], fp32 scale [rows] = absmax / 448)"""
    s = (x.float().abs().amax(1).clamp_min(1e-12) / 448.0).float()
    q = (x.float() / s[:, None]).clamp(-448.0, 448.0).to(F8)
    return q.view(torch.uint8), s


# ---- operand layouts -------------------------------------------------------------------------------------------------------------
def row_offsets(M, ld, rpb=0, bstride=0, device="cpu"):
    """element offset of the start of logical row m: m * ld, or under a row remap (m // rpb) * bstride + (m % rpb) * ld"""
    m = torch.arange(M, device=device, dtype=torch.int64)
    return m * ld if not rpb else (m // rpb) * bstride + (m % rpb) * ld


def gather_rows(buf, M, C, ld, rpb=0, bstride=0, base=0):
    """the [M, C] logical matrix the kernel reads out of the flat buffer `buf` from element `base` on"""
    idx = base + row_offsets(M, ld, rpb, bstride, buf.device)[:, None] + torch.arange(C, device=buf.device)
    return buf[idx]


# ---- class 1: operands whose every intermediate is exact -----------------------------------------------------------------------------
SPARSE_VALS = (1.0, -1.0, 2.0, -2.0)


def sparse_positions(rows, K, nnz=16):
    """[rows, nnz] K positions: nonzero j of row r sits in the j-th K / nnz block at an offset that moves with r and j"""
    blk = K // nnz
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    j = torch.arange(nnz, dtype=torch.int64)[None, :]
    return j * blk + (37 * r + 5 * j * j + 3 * j + (r // blk) * (2 * j + 1)) % blk


def sparse_int(rows, K, nnz=16):
    """uint8 [rows, K]: nnz nonzeros of +-1, +-2 per row"""
    pos = sparse_positions(rows, K, nnz)
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    j = torch.arange(nnz, dtype=torch.int64)[None, :]
    v = torch.zeros(rows, K)
    v.scatter_(1, pos, torch.tensor(SPARSE_VALS)[(r + j) % 4])
    return to_bytes(v)


def dense_int(rows, K, seed, dmax=8):
    """uint8 [rows, K]: integers of {-dmax .. dmax}, uniformly"""
    g = torch.Generator().manual_seed(seed)
    return to_bytes(torch.randint(-dmax, dmax + 1, (rows, K), generator=g).float())


GATE_VALS = (1.0, -1.0, 2.0, -2.0, 0.5)


def exact_operands(M, N, K, mirror, sub, ed, rpb=77):
    """class 1 operands (CPU). mirror "As": A sparse, W dense; "Ws": A dense, W sparse. sub "scale": power-of-two scales that vary
    with m and n, no bias; "epi": scales of 1, integer bias, gate out of GATE_VALS with rpb rows per batch, integer residual in the
    16-bit type, the dense operand in {-2 .. 2} so that |(acc + bias) * gate + R| <= 144 (a half-integer only below 43)."""
    seed = 1000003 * M + 1009 * N + K + (7 if mirror == "Ws" else 0)
    dmax = 8 if sub == "scale" else 2
    qa = sparse_int(M, K) if mirror == "As" else dense_int(M, K, seed, dmax)
    qw = dense_int(N, K, seed + 1, dmax) if mirror == "As" else sparse_int(N, K)
    o = dict(qa=qa, qw=qw, bias=None, gate=None, rpb=0, residual=None)
    if sub == "scale":
        o["sa"] = 2.0 ** -(torch.arange(M) % 5).float()
        o["sw"] = 2.0 ** (torch.arange(N) % 3 - 1).float()
    else:
        g = torch.Generator().manual_seed(seed + 2)
        o["sa"], o["sw"] = torch.ones(M), torch.ones(N)
        o["bias"] = torch.randint(-4, 5, (N,), generator=g).float()
        nb = (M + rpb - 1) // rpb
        o["gate"] = torch.tensor(GATE_VALS)[torch.randint(0, len(GATE_VALS), (nb, N), generator=g)]
        o["rpb"] = rpb
        o["residual"] = torch.randint(-8, 9, (M, N), generator=g).float().to(ed)
    return o


def exact_q_operands(o):
    """adds the e4m3 output's operands to class 1 operands: a_l2 = the row norm of A times a factor in [2, 2.9) that moves
    irregularly with m, w_norm_max = the largest row norm of W (Cauchy-Schwarz: nothing saturates), bias_abs_max = 0. Without the
    factor the few values y / s of this class repeat down the rows, and one that falls next to a rounding tie does so everywhere."""
    A = from_bytes(o["qa"]) * o["sa"].double()[:, None]
    W = from_bytes(o["qw"]) * o["sw"].double()[:, None]
    m = torch.arange(A.shape[0], dtype=torch.float64, device=A.device)
    o["a_l2"] = (A.norm(dim=1) * (2.0 + 0.9 * torch.frac((m + 1) * 0.7548776662466927))).float()
    o["w_norm_max"], o["bias_abs_max"] = float(W.norm(dim=1).max().float()), 0.0
    return o


def exact_reference(o, ed):
    """float64 value of a class 1 case, with the precondition asserted: it is its own rounding to ed"""
    ref, _ = reference8(o["qa"], o["sa"], o["qw"], o["sw"], bias=o["bias"], gate=o["gate"], rows_per_batch=o["rpb"],
                        residual=o["residual"])
    assert torch.equal(ref.to(ed).double(), ref), "class 1 precondition: the reference is not exact in the 16-bit type"
    return ref


def exact_off(out, ref):
    """number of elements of the 16-bit output whose bits differ from ref.to(out.dtype)"""
    return BP.exact_off(out, ref.to(out.dtype))


# ---- class 2: dense operands at realistic magnitudes ---------------------------------------------------------------------------------
def dense_operands(M, N, K, form, ed, rpb=77):
    """class 2 operands (CPU), quantised as the model does. Row magnitudes of A vary by 4x, W row 1 is 40x larger. form: a subset of
    "bias", "gate" (+ residual, rpb rows per batch), "gelu" joined by "+" ("" = none). Also the operands of the e4m3 output: a_l2
    (the row norms before quantisation), w_norm_max, bias_abs_max (both fp32 values)."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    a = (torch.randn(M, K, generator=g) + 0.5) * (1 + 3 * torch.rand(M, 1, generator=g))
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    # the large row is non-negative and A has a row mean of half a sigma, so its channel is positive (0.4 sqrt(K) sigmas): under
    # GELU a large NEGATIVE value is ~0 with the Lipschitz bound of a large value around it -- an interval of several subnormal
    # codes on half of that channel, 1 / (2 N) of a narrow case's elements, which alone would exceed MULTI_CAP at N = 8
    w[min(1, N - 1)] = 40.0 * w[min(1, N - 1)].abs()
    qa, sa = quantize_rows(a)
    qw, sw = quantize_rows(w)
    bias = torch.randn(N, generator=g) * 0.1
    nb = (M + rpb - 1) // rpb
    gate = torch.randn(nb, N, generator=g)
    residual = torch.randn(M, N, generator=g).to(ed)
    parts = set(form.split("+")) - {""}
    o = dict(qa=qa, sa=sa, qw=qw, sw=sw, bias=bias if "bias" in parts or "gate" in parts else None,
             gate=gate if "gate" in parts else None, rpb=rpb if "gate" in parts else 0,
             residual=residual if "gate" in parts else None, gelu="gelu" in parts)
    o["a_l2"] = a.norm(dim=1).float()
    o["w_norm_max"] = float((from_bytes(qw) * sw.double()[:, None]).norm(dim=1).max().float())
    o["bias_abs_max"] = float(bias.abs().max()) if o["bias"] is not None else 0.0
    return o


def reference8(qa, sa, qw, sw, *, bias=None, gate=None, rows_per_batch=0, residual=None, gelu=False):
    """float64 reference and elementwise error e (before the output rounding) of
    act(((qa sa) @ (qw sw)^T + bias) * gate[m // rows_per_batch] + residual): the W8A8 counterpart of gemm_bounds.reference.
    qa [M, K], qw [N, K] uint8 e4m3 bytes; sa [M], sw [N] fp32; bias [N]; gate [batches, N]; residual [M, N] 16-bit."""
    M, K = qa.shape
    A = from_bytes(qa) * sa.double()[:, None]
    W = from_bytes(qw) * sw.double()[:, None]
    acc = A @ W.t()
    e = gamma8(K) * (A.abs() @ W.abs().t())
    del A, W
    b = bias.double() if bias is not None else torch.zeros(acc.shape[1], dtype=torch.float64, device=acc.device)
    z, mag = acc + b, acc.abs() + b.abs()
    del acc
    if gate is not None:
        g = gate.double()[torch.arange(M, device=z.device) // rows_per_batch]
        z, e, mag = z * g, e * g.abs(), mag * g.abs()
    if residual is not None:
        r = residual.double()
        z, mag = z + r, mag + r.abs()
    e = e + EPI_OPS8 * U32 * mag
    if gelu:
        e = GB.SLOPE["gelu_tanh"] * e + GB.ACT_REL * z.abs()
        z = GB._act("gelu_tanh", z)
    return z, e


# ---- e4m3 output -----------------------------------------------------------------------------------------------------------------
F32_1P1 = float(torch.tensor(1.1, dtype=torch.float32).double())


def out_scale64(a_l2, w_norm_max, bias_abs_max):
    """s64 [M]: the row scale of mi355x_sd_linear_f8_q in float64, from the fp32 operands as the kernel receives them"""
    f = lambda v: float(torch.tensor(v, dtype=torch.float32).double())   # noqa: E731  (c_float arguments)
    return F32_1P1 * (a_l2.double() * f(w_norm_max) + f(bias_abs_max)) / 448.0


def interval(ref, e, s):
    """(lo, hi) e4m3 values (float64) of the accepted codes of every element; s [M] the row scale the bytes are judged with"""
    ep = e + 8 * U32 * ref.abs()
    sd = s.double()[:, None]
    return e4m3_round((ref - ep) / sd), e4m3_round((ref + ep) / sd)


def multi_share(ref, e, s):
    """share of elements whose interval holds more than one code"""
    lo, hi = interval(ref, e, s)
    return (lo != hi).double().mean().item()


def check_q(q, c_scale, ref, e, s64):
    """the e4m3 output q [M, N] (uint8) with its row scales c_scale [M] (fp32) -> dict(scale_ratio: worst |c_scale - s64| / (4 2^-24
    s64); outside: bytes outside their interval; nan: NaN bytes; multi: share of intervals with more than one code)"""
    cs = c_scale.double()
    sr = ((cs - s64).abs() / (4 * U32 * s64)).max().item()
    if sr != sr or not torch.isfinite(cs).all():
        sr = float("inf")
    lo, hi = interval(ref, e, c_scale)
    v = from_bytes(q)
    nan = (q & 0x7F) == 0x7F
    outside = (~((v >= lo) & (v <= hi))) & ~nan
    return dict(scale_ratio=sr, outside=int(outside.sum().item()), nan=int(nan.sum().item()),
                multi=(lo != hi).double().mean().item())


# ---- fp32 emulation of the kernel, with planted mistakes ----------------------------------------------------------------------------
FAULTS = ("swap_chunks_a", "drop_last_ktile", "a_scale_next_row", "clamped_column", "bias_twice", "gate_by_subtile",
          "residual_before_gate", "a_remap_no_stride", "no_1p1", "e4m3_toward_zero")


def _gelu_tanh_f32(x):
    u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
    return x / (1.0 + torch.exp(-2.0 * u))


def emulate(qa, sa, qw, sw, ed, *, bias=None, gate=None, rows_per_batch=0, residual=None, gelu=False, a_remap=None, q=None,
            fault=None):
    """fp32 restatement of gemm256_kernel<F8> + gemm_epilogue_f8 -> the 16-bit output [M, N], or with q = dict(a_l2, w_norm_max,
    bias_abs_max) the e4m3 output (uint8 [M, N], fp32 c_scale [M]). a_remap = dict(M, lda, rpb, bstride, base): qa is the flat
    byte buffer the rows are read from. fault: one of FAULTS, the planted mistake."""
    assert fault is None or fault in FAULTS, fault
    if a_remap is not None:
        r = dict(a_remap)
        if fault == "a_remap_no_stride":   # the batch stride ignored: rows taken as if the segments were adjacent
            r["bstride"] = r["rpb"] * r["lda"]
        qa = gather_rows(qa, r["M"], qw.shape[1], r["lda"], r["rpb"], r["bstride"], r.get("base", 0))
    M, K = qa.shape
    N = qw.shape[0]
    A, W = qa.view(F8).float(), qw.view(F8).float()
    if fault == "swap_chunks_a":           # a lane's fragment pair: the 16-byte chunks 2 fkc, 2 fkc + 1 exchanged
        A = A[:, torch.arange(K) ^ 16]
    nt = K // KT - (1 if fault == "drop_last_ktile" else 0)
    acc = torch.zeros(M, N)
    for t in range(nt):                    # one 128-deep step per K-tile, chained in fp32
        acc = acc + A[:, t * KT:(t + 1) * KT] @ W[:, t * KT:(t + 1) * KT].t()
    m = torch.arange(M)
    as_ = sa.float()[(m + 1).clamp(max=M - 1)] if fault == "a_scale_next_row" else sa.float()
    ws, b = sw.float().clone(), None if bias is None else bias.float().clone()
    if fault == "clamped_column" and N % 8 == 4 and N >= 8:   # the last group's per-channel operands from one group to the left
        ws[N - 4:] = ws[N - 8:N - 4].clone()
        if b is not None:
            b[N - 4:] = b[N - 8:N - 4].clone()
    v = acc * as_[:, None] * ws[None, :]
    if b is not None:
        v = v + b
        if fault == "bias_twice":
            v = v + b
    rf = None if residual is None else residual.float()
    if rf is not None and fault == "residual_before_gate":
        v = v + rf
    if gate is not None:
        gi = (m // 16 * 16 // rows_per_batch) if fault == "gate_by_subtile" else m // rows_per_batch
        v = v * gate.float()[gi]
    if rf is not None and fault != "residual_before_gate":
        v = v + rf
    if gelu:
        v = _gelu_tanh_f32(v)
    if q is None:
        return v.to(ed)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    bound = (f32(1.0) if fault == "no_1p1" else f32(1.1)) * (q["a_l2"].float() * f32(q["w_norm_max"]) + f32(q["bias_abs_max"]))
    bound = bound.clamp_min(1e-12)
    oinv = f32(448.0) / bound
    cs = bound * (f32(1.0) / f32(448.0))
    y = v * oinv[:, None]
    if fault == "e4m3_toward_zero":
        return to_bytes(e4m3_round(y.double(), toward_zero=True)), cs
    return y.clamp(-448.0, 448.0).to(F8).view(torch.uint8), cs
