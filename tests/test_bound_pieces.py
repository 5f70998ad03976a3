"""CPU: every kernel family's check() returns, float for float, what its own formula gives. The formulas are restated here by hand,
element by element in Python floats (IEEE doubles, the operations in the order each family's module had them before the families
shared tests/bound_pieces.py), on the family's own reference() at a small shape and on the edge cases a shared comparison could get
wrong: an element with ref = e = err = 0, one with a zero bound and an error, a NaN in the output, a zero reference tensor.
Also exact_off() over 1-, 2- and 4-byte elements."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests import attn_cases as AC
from tests import bound_pieces as BP
from tests import conv_bounds as CB
from tests import freeu_bounds as UB
from tests import gemm_bounds as GB
from tests import gemm_f8_bounds as FB
from tests import norm_bounds as NB
from tests import rowmap_bounds as RB

U = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
U32 = 2.0 ** -24
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


# ---- the formulas, by hand ----------------------------------------------------------------------------------------------------------
def _ratio(out, ref, e, bound_of, zero_pass):
    worst = 0.0
    for o, r, ee in zip(out.double().flatten().tolist(), ref.flatten().tolist(), e.flatten().tolist()):
        err, bound = abs(o - r), bound_of(r, ee)
        if zero_pass and bound == 0 and err == 0:
            continue
        q = err / bound if bound != 0 else (math.nan if err == 0 or err != err else math.inf)
        if q != q or not math.isfinite(o):
            return math.inf
        worst = max(worst, q)
    return worst


def _rel(out, ref, floor):
    den = ref.norm()
    return ((out.double() - ref).norm() / (den.clamp_min(floor) if floor else den)).item()


def b16(u):
    return lambda r, e: u * abs(r) + (1 + u) * e + U32


def want_gemm(out, ref, e):        # gemm_bounds, conv_bounds, gemm_f8: fp32 = the epilogue value, 0 / 0 passes; rel-L2 unclamped
    if out.dtype == F32:
        return _ratio(out, ref, e, lambda r, ee: ee + U32 * abs(r), True), _rel(out, ref, 0)
    return _ratio(out, ref, e, b16(U[out.dtype]), False), _rel(out, ref, 0)


def want_attn(out, ref, e):        # 16-bit only; rel-L2's denominator clamped at 1e-300
    return _ratio(out, ref, e, b16(U[out.dtype]), False), _rel(out, ref, 1e-300)


def want_norm(out, ref, e, u_out=None):   # one form for every dtype: fp32 is u = 0 WITH the 2^-24 floor; clamped
    u = (0.0 if out.dtype == F32 else U[out.dtype]) if u_out is None else u_out
    return _ratio(out, ref, e, b16(u), False), _rel(out, ref, 1e-300)


def want_rowmap(out, ref, e):      # rowmap_bounds, freeu_bounds: fp32 rounds once more, 0 / 0 passes; the ratio alone
    if out.dtype == F32:
        return _ratio(out, ref, e, lambda r, ee: 2 * U32 * abs(r) + ee, True)
    return _ratio(out, ref, e, b16(U[out.dtype]), True)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _edges(dt):
    """(label, out, ref, e): the edge cases, on 8 elements"""
    ref = torch.tensor([0.0, 0.0, 1.0, -2.5, 3.0, 0.125, -7.0, 0.5], dtype=torch.float64)
    e = torch.tensor([0.0, 0.0, 1e-3, 2e-3, 0.0, 1e-4, 0.0, 1e-5], dtype=torch.float64)
    exact = ref.to(dt)                                   # err = 0 everywhere, elements 0 and 1 with ref = e = 0
    off = ref.clone()
    off[1] = 2.0 ** -10                                  # ref = e = 0 and an error: a zero bound wherever there is no floor
    nan = ref.clone()
    nan[3] = math.nan
    inf = ref.clone()
    inf[6] = math.inf
    zero = torch.zeros(8, dtype=torch.float64)
    return [("exact", exact, ref, e), ("zero bound", off.to(dt), ref, e), ("nan", nan.to(dt), ref, e), ("inf", inf.to(dt), ref, e),
            ("zero ref", zero.to(dt), zero, zero), ("zero ref, error", (zero + 0.25).to(dt), zero, zero),
            ("near", (ref * (1 + 2.0 ** -9) + 1e-4).to(dt), ref, e)]


def _noisy(ref, e, dt, seed):
    """a reference with a plausible output: the reference rounded to dt after an error of about e"""
    g = torch.Generator().manual_seed(seed)
    return (ref + e * (2 * torch.rand(ref.shape, generator=g, dtype=torch.float64) - 1)).to(dt)


def _family_inputs(family):
    g = torch.Generator().manual_seed(11)
    if family in ("gemm", "conv", "f8"):
        if family == "gemm":
            a, w = torch.randn(5, 64, generator=g).to(BF), torch.randn(4, 64, generator=g).to(BF)
            ref, e = GB.reference(a, w, bias=torch.randn(4, generator=g), act="silu")
        elif family == "conv":
            x, w = torch.randn(1, 2, 3, 8, generator=g).to(BF), torch.randn(4, 72, generator=g).to(BF)
            ref, e = CB.conv3x3_reference(x, w, bias=torch.randn(4, generator=g))
        else:
            o = FB.dense_operands(3, 4, 128, "bias", BF)
            ref, e = FB.reference8(o["qa"], o["sa"], o["qw"], o["sw"], bias=o["bias"])
        return [(f"{family} {dt}", _noisy(ref, e, dt, 1), ref, e) for dt in (BF, HF, F32)]
    if family == "attn":
        c = AC.make(dict(B=1, H=2, Sq=3, Skv=5, D=8, kind="S4", bias=None, log2=False, accum=None, ninf=False), HF, seed=3)
        ref, e = AB.reference(c["q"], c["k"], c["v"], scale=c["scale"])
        return [(f"attn {dt}", _noisy(ref, e, dt, 2), ref, e) for dt in (BF, HF)]
    if family == "norm":
        x = torch.randn(3, 64, generator=g).to(HF)
        ref, e = NB.layernorm(x, None, None, 1e-5, NB.chain_rows("layernorm", 1024))
        rs, es = NB.row_stats(x, 1e-5, NB.chain_rows("row_stats", 1024))
        return [(f"norm {dt}", _noisy(ref, e, dt, 3), ref, e) for dt in (BF, HF, F32)] + [("norm row_stats", _noisy(rs, es, F32, 4), rs, es)]
    x = torch.randn(40, generator=g)
    if family == "freeu":
        ref, e = RB.act("silu", x.double())
    else:
        ref, e = RB.axpby(x, torch.randn(40, generator=g), torch.tensor([1.5, -0.25]))
    return [(f"{family} {dt}", _noisy(ref, e, dt, 5), ref, e) for dt in (BF, HF, F32)]


FAMILIES = {"gemm": (GB.check, want_gemm, (BF, HF, F32)), "conv": (CB.check, want_gemm, (BF, HF, F32)),
            "f8": (GB.check, want_gemm, (BF, HF)), "attn": (AB.check, want_attn, (BF, HF)),
            "norm": (NB.check, want_norm, (BF, HF, F32)), "rowmap": (RB.check, want_rowmap, (BF, HF, F32)),
            "freeu": (UB.check, want_rowmap, (BF, HF, F32))}


def _same(got, want):
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    return len(got) == len(want) and all(a == b or (a != a and b != b) for a, b in zip(got, want))   # (== on floats; NaN is NaN)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_check_is_its_own_formula(family):
    check, want, dts = FAMILIES[family]
    cases = _family_inputs(family) + [(f"{lab} {dt}", o, r, e) for dt in dts for lab, o, r, e in _edges(dt)]
    for label, out, ref, e in cases:
        got, exp = check(out, ref, e), want(out, ref, e)
        print(f"{family:<7} {label:<32} {got}")
        assert _same(got, exp), (family, label, got, exp)


def test_norm_check_takes_an_explicit_u_out():
    for lab, out, ref, e in _edges(F32) + _edges(HF):
        for u in (0.0, 2.0 ** -8):
            assert _same(NB.check(out, ref, e, u_out=u), want_norm(out, ref, e, u)), (lab, u)


def test_the_conventions_that_differ_stay_different():
    """fp32 stores: 2^-24 |ref| (GEMM, convolution), 2 * 2^-24 |ref| (row maps), u = 0 with the 2^-24 floor (normalisation).
    rel-L2 of a zero reference: NaN where the denominator is left alone, 0 or a huge number where it is clamped."""
    ref, e = torch.tensor([1.0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    out = torch.tensor([1.0 + 2.0 ** -23], dtype=F32)   # one fp32 ulp off
    assert GB.check(out, ref, e)[0] == 2.0 and RB.check(out, ref, e) == 1.0 and NB.check(out, ref, e)[0] == 2.0
    zero = torch.zeros(4, dtype=torch.float64)
    assert math.isnan(GB.check(zero.to(BF), zero, zero)[1]) and AB.check(zero.to(BF), zero, zero)[1] == 0.0
    assert NB.check(zero.to(BF), zero, zero)[1] == 0.0
    assert GB.check(zero.float(), zero, zero)[0] == 0.0 and RB.check(zero.float(), zero, zero) == 0.0   # 0 / 0 passes
    assert GB.check(zero.float() + 1, zero, zero)[0] == math.inf and RB.check(zero.float() + 1, zero, zero) == math.inf


def test_shared_constants_are_the_families():
    for m in (GB, AB, NB, RB):
        assert m.U32 == BP.U32 == 2.0 ** -24
        assert m.U_OUT[BF] == 2.0 ** -7 and m.U_OUT[HF] == 2.0 ** -10
    assert NB.U_OUT[F32] == 0.0 and F32 not in BP.U_OUT
    for x in (0.1, 1e-5, 1.0 / math.sqrt(40), 0.18215):
        assert AB.fp32(x) == NB.fp32(x) == BP.fp32(x) == float(torch.tensor(x, dtype=F32).double())


def test_exact_off_counts_differing_elements():
    for dt in (torch.uint8, BF, HF, F32, torch.int32):
        a = torch.arange(24).reshape(4, 6).to(dt)
        b = a.clone()
        assert BP.exact_off(a, b) == 0
        b[1, 2] += 1
        b[3, 5] += 1
        assert BP.exact_off(a, b) == 2 and BP.exact_off(a.t(), b.t()) == 2   # (non-contiguous views too)
        assert BP.exact_off(a, a[:3]) == 24 and BP.exact_off(a[:3], a) == 24    # a shape mismatch: every element
    a = torch.zeros(5, dtype=HF)
    assert BP.exact_off(a, a.to(BF)) == 5                                       # a dtype mismatch: every element
    assert BP.exact_off(a, -a) == 5                                             # bits, not values: -0 is not +0
    n = torch.full((3,), math.nan)
    assert BP.exact_off(n, n.clone()) == 0                                      # ... and a NaN equals itself
    assert RB.exact_off(a, -a) == 5
    ref = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    assert FB.exact_off(ref.to(HF), ref) == 0 and FB.exact_off((ref + 1).to(HF), ref) == 3   # (gemm_f8: against ref rounded to out's type)
