"""The elementwise fp64 bound of tests/gemm_bounds.py, checked on the CPU: it accepts an emulation of the kernels' arithmetic (16-bit
operands, fp32 sums of 32-deep chunks, one rounding of the result) and rejects that emulation with one element off by four output
ulps, with one 32-deep K chunk missing from one 16 x 16 sub-tile, and with the bias added twice."""
import pytest
import torch

from tests import gemm_bounds as GB

M, N, K = 96, 96, 320


def _operands(dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dt)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    b = torch.randn(N, generator=g)
    return a, w, b


def _emulate(a, w, b, dt, drop_chunk=None, bias_times=1):
    """fp32 accumulators over 32-deep chunks (each chunk's sum rounded to fp32 once, as one MFMA step), bias in fp32, one 16-bit
    rounding. drop_chunk = (row0, col0, chunk): that chunk is left out of the 16 x 16 sub-tile at (row0, col0)."""
    af, wf = a.double(), w.double()
    acc = torch.zeros(M, N, dtype=torch.float32)
    for c in range(K // 32):
        part = (af[:, 32 * c:32 * c + 32] @ wf[:, 32 * c:32 * c + 32].t()).float()
        if drop_chunk is not None and drop_chunk[2] == c:
            r0, c0 = drop_chunk[:2]
            part[r0:r0 + 16, c0:c0 + 16] = 0
        acc = acc + part
    for _ in range(bias_times):
        acc = acc + b
    return acc.to(dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bound_accepts_the_kernel_arithmetic(dt):
    a, w, b = _operands(dt)
    ratio, rel = GB.bound_check(_emulate(a, w, b, dt), a, w, bias=b)
    assert ratio < 0.75, ratio   # (one 16-bit rounding: at most half of u_out, plus the accumulation's share)
    assert rel < (4e-3 if dt == torch.bfloat16 else 6e-4), rel


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bound_rejects_one_element_four_ulps_off(dt):
    a, w, b = _operands(dt)
    out = _emulate(a, w, b, dt)
    i = out.float().abs().argmax()
    x = out.view(-1)[i].float()
    ulp = (torch.nextafter(x.to(dt), torch.tensor(float("inf"), dtype=dt)).float() - x).abs()
    bad = out.clone()
    bad.view(-1)[i] = (x + 4 * ulp * x.sign()).to(dt)
    assert (bad.float() - out.float()).abs().max() == 4 * ulp
    ratio, _ = GB.bound_check(bad, a, w, bias=b)
    assert ratio > 1.5, ratio


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bound_rejects_a_dropped_k_chunk_in_one_sub_tile(dt):
    a, w, b = _operands(dt)
    ratio, rel = GB.bound_check(_emulate(a, w, b, dt, drop_chunk=(48, 32, 3)), a, w, bias=b)
    assert ratio > 4, ratio
    assert rel < 4e-2   # (rel-L2 of the whole output hardly notices: the reason for the elementwise bound)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bound_rejects_the_bias_added_twice(dt):
    a, w, b = _operands(dt)
    ratio, _ = GB.bound_check(_emulate(a, w, b, dt, bias_times=2), a, w, bias=b)
    assert ratio > 4, ratio


def test_bound_accepts_the_epilogue_forms():
    """gate + residual + out_scale, SiLU, tanh-GELU and GEGLU (interleaved 16 value | 16 gate columns) in fp32 after the emulated
    accumulator, against the reference's float64 forms: inside the bound; the activation's slope constants cover the functions"""
    dt = torch.bfloat16
    a, w, b = _operands(dt, 1)
    acc = _emulate(a, w, torch.zeros(N), torch.float32)   # (fp32 accumulators, not rounded to 16 bits)
    z = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    for name, L in GB.SLOPE.items():
        zz = z.clone().requires_grad_(True)
        GB._act(name, zz).sum().backward()
        assert zz.grad.abs().max().item() < L, name
    g = torch.Generator().manual_seed(2)
    gate = torch.randn(3, N, generator=g)
    r = torch.randn(M, N, generator=g).to(dt)
    out = (((acc + b) * gate[torch.arange(M) // 32] + r.float()) * 0.7).to(dt)
    assert GB.bound_check(out, a, w, bias=b, gate=gate, rows_per_batch=32, residual=r, out_scale=0.7)[0] < 0.75
    for act, f in (("silu", torch.nn.functional.silu), ("gelu_tanh", lambda v: torch.nn.functional.gelu(v, approximate="tanh"))):
        assert GB.bound_check(f(acc + b).to(dt), a, w, bias=b, act=act)[0] < 0.75, act
    y = (acc + b).reshape(M, N // 32, 2, 16)
    out = (y[:, :, 0] * torch.nn.functional.gelu(y[:, :, 1])).reshape(M, N // 2).to(dt)
    assert GB.bound_check(out, a, w, bias=b, geglu=True)[0] < 0.75
    # the GEGLU halves swapped (value <-> gate): far outside
    out_sw = (torch.nn.functional.gelu(y[:, :, 0]) * y[:, :, 1]).reshape(M, N // 2).to(dt)
    assert GB.bound_check(out_sw, a, w, bias=b, geglu=True)[0] > 4


# ---- the forms of the linear launches (tests/test_gpu_gemm_linear.py): LayerNorm fold, row bias, fp32 residual stream, split-K, +f8 ----
DTS = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
RPB = 77   # (the SD3 context length: with M = 96 the batch boundary falls inside the 16-row sub-tile of rows 64 .. 79)


def _acc32(a, w, slices=1, drop=None):
    """fp32 accumulators of a @ w^T as the kernels sum them: 32-deep chunks in a chain, each rounded to fp32 once. slices > 1: the
    chunks in `slices` contiguous groups (the last may be shorter), each its own chain from zero, the group sums added in index order
    (split-K slices + splitk_reduce_kernel). drop = (row0, col0, slice): that slice is missing from the 16 x 16 sub-tile."""
    af, wf = a.double(), w.double()
    nc = a.shape[1] // 32
    per = -(-nc // slices)
    tot = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for s in range(slices):
        acc = torch.zeros_like(tot)
        for c in range(s * per, min(nc, (s + 1) * per)):
            acc = acc + (af[:, 32 * c:32 * c + 32] @ wf[:, 32 * c:32 * c + 32].t()).float()
        if drop is not None and drop[2] == s:
            acc[drop[0]:drop[0] + 16, drop[1]:drop[1] + 16] = 0
        tot = tot + acc if slices > 1 else acc
    return tot


def _ln_operands(dt, seed=3):
    """activations with a row mean several times the row deviation (as test_layernorm_folded_linear: the correction term cancels a
    large common component), their exact statistics rounded to fp32 once, folded weights and their fp32 row sums"""
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 0.5 + torch.randn(M, 1, generator=g) * 3.0).to(dt)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    b = torch.randn(N, generator=g) * 0.1
    mean, var = a.double().mean(1), a.double().var(1, unbiased=False)
    assert (mean.abs() / var.sqrt()).median() > 3
    rstd = torch.rsqrt(var + 1e-5)
    st = torch.stack([rstd, -mean * rstd], 1).float()
    return a, w, b, st, w.float().sum(1)


def _ln_epilogue(acc, st, wsum, b, dt, use_wsum=True, swap=False):
    r, n = (st[:, 1:], st[:, :1]) if swap else (st[:, :1], st[:, 1:])
    v = r * acc
    if use_wsum:
        v = v + n * wsum
    return (v + b).to(dt)


@DTS
def test_bound_accepts_the_layernorm_fold_and_rejects_a_missing_or_swapped_term(dt):
    a, w, b, st, wsum = _ln_operands(dt)
    acc = _acc32(a, w)
    kw = dict(bias=b, rowstat=st, wsum=wsum)
    ratio, rel = GB.bound_check(_ln_epilogue(acc, st, wsum, b, dt), a, w, **kw)
    assert ratio < 0.75, ratio
    assert rel < (4e-3 if dt == torch.bfloat16 else 6e-4), rel
    assert GB.bound_check(_ln_epilogue(acc, st, wsum, b, dt, use_wsum=False), a, w, **kw)[0] > 4
    assert GB.bound_check(_ln_epilogue(acc, st, wsum, b, dt, swap=True), a, w, **kw)[0] > 4
    # GEGLU behind the fold (interleaved 16 value | 16 gate columns)
    y = (st[:, :1] * acc + st[:, 1:] * wsum + b).reshape(M, N // 32, 2, 16)
    out = (y[:, :, 0] * torch.nn.functional.gelu(y[:, :, 1])).reshape(M, N // 2).to(dt)
    assert GB.bound_check(out, a, w, geglu=True, **kw)[0] < 0.75


def _batched(v, wrong):
    """per-row operand v[m // RPB]; wrong: the rows of the sub-tile 64 .. 79 all take the batch of its first row, so rows 77 .. 79
    read the neighbouring batch"""
    idx = torch.arange(M) // RPB
    if wrong:
        idx[64:80] = 64 // RPB
    return v[idx]


@DTS
def test_bound_accepts_rowbias_and_gate_and_rejects_the_neighbouring_batch_in_one_sub_tile(dt):
    a, w, b = _operands(dt, 4)
    acc = _acc32(a, w)
    g = torch.Generator().manual_seed(5)
    rb, gate = torch.randn(2, N, generator=g), torch.randn(2, N, generator=g)
    r = torch.randn(M, N, generator=g).to(dt)
    for wrong in (False, True):
        out = ((acc + b + _batched(rb, wrong) + r.float()) * 0.7).to(dt)
        ratio, _ = GB.bound_check(out, a, w, bias=b, rowbias=rb, rows_per_batch=RPB, residual=r, out_scale=0.7)
        assert (ratio > 4) if wrong else (ratio < 0.75), ("rowbias", wrong, ratio)
        out = ((acc + b) * _batched(gate, wrong) + r.float()).to(dt)
        ratio, _ = GB.bound_check(out, a, w, bias=b, gate=gate, rows_per_batch=RPB, residual=r)
        assert (ratio > 4) if wrong else (ratio < 0.75), ("gate", wrong, ratio)


@DTS
def test_bound_accepts_the_fp32_residual_stream(dt):
    """fp32 residual rows in, the fp32 sum out (R_F32 | OUT_F32): no output rounding, the bound is e + 2^-24 |ref|"""
    a, w, b = _operands(dt, 6)
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(7))
    out = _acc32(a, w) + b + r
    assert out.dtype == torch.float32
    ratio, rel = GB.bound_check(out, a, w, bias=b, residual=r)
    assert ratio < 0.75 and rel < 1e-6, (ratio, rel)
    bad = _emulate(a, w, b, torch.float32, drop_chunk=(48, 32, 3)) + r   # (one 32-deep chunk missing from one sub-tile)
    assert GB.bound_check(bad, a, w, bias=b, residual=r)[0] > 4


@DTS
def test_bound_accepts_split_k_slices_and_rejects_a_missing_slice_in_one_sub_tile(dt):
    """K = 1024: 16 K-tiles in four slices of four (plan_splitk's shortest slice), and in three uneven ones (6 + 6 + 4)"""
    g = torch.Generator().manual_seed(8)
    Kd = 1024
    a = torch.randn(M, Kd, generator=g).to(dt)
    w = (torch.randn(N, Kd, generator=g) / Kd ** 0.5).to(dt)
    b = torch.randn(N, generator=g)
    for s in (4, 3):
        ratio, _ = GB.bound_check((_acc32(a, w, slices=s) + b).to(dt), a, w, bias=b)
        assert ratio < 0.75, (s, ratio)
        ratio, rel = GB.bound_check((_acc32(a, w, slices=s, drop=(48, 32, s - 1)) + b).to(dt), a, w, bias=b)
        assert ratio > 4, (s, ratio)
        assert rel < 4e-2 * 4   # (a quarter to a third of the sum in 256 of 9216 elements: the rel-L2 bar's order of magnitude)


@DTS
def test_bound_accepts_in_kernel_e4m3_weights_and_rejects_the_scale_after_the_bias(dt):
    """+f8: exact e4m3 fragments, acc * scale, then the bias (gemm_epilogue.h epi4). Reference weights: Q * scale in float64."""
    g = torch.Generator().manual_seed(9)
    a = torch.randn(M, K, generator=g).to(dt)
    wf = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    scale = (wf.abs().amax(1) / 448.0).float()
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn).float()
    acc = _acc32(a, q)
    w_ref = q.double() * scale.double()[:, None]
    assert GB.bound_check((acc * scale + b).to(dt), a, w_ref, bias=b)[0] < 0.75
    assert GB.bound_check(((acc + b) * scale).to(dt), a, w_ref, bias=b)[0] > 4
    # bias in the accumulators (bias_acc): the chain starts at the bias instead of zero
    a2, w2, b2 = _operands(dt, 10)
    chain = b2.expand(M, N).clone()
    for c in range(K // 32):
        chain = chain + (a2.double()[:, 32 * c:32 * c + 32] @ w2.double()[:, 32 * c:32 * c + 32].t()).float()
    assert GB.bound_check(chain.to(dt), a2, w2, bias=b2, bias_acc=True)[0] < 0.75
