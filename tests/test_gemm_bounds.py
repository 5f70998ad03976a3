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
