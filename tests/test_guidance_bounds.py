"""The bound of tests/guidance_bounds.py, checked on the CPU: the fp32 restatement of the device kernel in its own order
(tests/abi_emulator_guidance.py emulate) stays under it on every case the GPU test runs, the float64 reference itself sits orders
of magnitude inside it against an extended-precision evaluation, and a deliberately wrong emulation -- the variance in one fp32
pass, sum v^2 - n mean^2 -- lands far above it on the case built to expose it (values 64 + 1e-2 N(0, 1)). Ratios are printed
(pytest -s)."""
import numpy as np
import pytest
import torch

from tests import guidance_bounds as GB
from tests import rowmap_bounds as RB
from tests.abi_emulator_guidance import emulate, tree_sum

OFFSET = "b2 n4092 offset 64"


@pytest.mark.parametrize("name", list(GB.CASES))
def test_emulation_inside_the_bound(name):
    x, eu, et, coef, gs, gr = GB.inputs(name)
    ref, e, _ = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr)
    assert torch.isfinite(e).all()
    ratio = RB.check(emulate(x, eu, et, coef, gs, gr), ref, e)
    print(f"{name:<28} err/bound {ratio:.3f}")
    assert ratio < 1.0


def _extended(x, eu, et, coef, gs, gr):
    """the same quantity in numpy's extended precision, organised differently (np.std on mean-free data)"""
    ld = np.longdouble
    a, b = (ld(v) for v in coef.double().tolist())
    xx, u, t = (v.double().numpy().astype(ld) for v in (x, eu, et))
    c = u + ld(np.float32(gs)) * (t - u)
    r = np.std(t - t.mean(1, keepdims=True), axis=1, ddof=1, keepdims=True) / np.std(c - c.mean(1, keepdims=True), axis=1, ddof=1, keepdims=True)
    g = ld(np.float32(gr))
    return a * xx + b * c * (g * r + (1 - g))


def test_reference_is_well_inside_the_bound_and_one_pass_variance_is_outside():
    x, eu, et, coef, gs, gr = GB.inputs(OFFSET)
    ref, e, _ = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr)
    bound = 2 * RB.U32 * ref.abs() + e
    own = float(np.max(np.abs(ref.numpy().astype(np.longdouble) - _extended(x, eu, et, coef, gs, gr)) / bound.numpy()))
    good = RB.check(emulate(x, eu, et, coef, gs, gr), ref, e)
    bad = RB.check(emulate(x, eu, et, coef, gs, gr, variance="one_pass"), ref, e)
    print(f"offset case: float64 reference vs extended precision {own:.2e} of the bound; two-pass emulation {good:.3f}; "
          f"one-pass fp32 variance {bad:.3g} (bound / |ref| at most {float((bound / ref.abs()).max()):.2e})")
    assert own < 1e-3
    assert good < 1.0
    assert bad > 1.0


def test_one_pass_variance_is_invisible_without_an_offset():
    """(why the offset case exists: on mean-free inputs the wrong form passes)"""
    x, eu, et, coef, gs, gr = GB.inputs("b3 n4092 ragged")
    ref, e, _ = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr)
    bad = RB.check(emulate(x, eu, et, coef, gs, gr, variance="one_pass"), ref, e)
    print(f"one-pass variance on mean-free inputs: err/bound {bad:.3f}")
    assert bad < 1.0


def test_special_cases_of_the_bound():
    # gr = 0: k is exactly 1 and the reference and bound are cfg_axpby's own
    x, eu, et, coef, gs, gr = GB.inputs("b2 n4096 gr0")
    ref, e, _ = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr)
    ref0, e0 = RB.cfg_axpby(x, eu, et, coef, gs)
    assert torch.equal(ref, ref0)
    assert RB.check(emulate(x, eu, et, coef, gs, gr), ref0, e0) < 1.0
    # gr = 1, gs = 1: c = et and r = 1 up to rounding: out = a x + b et
    x, eu, et, coef, gs, gr = GB.inputs("b2 n4096 gr1 gs1")
    ref, e, ck = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr)
    assert torch.allclose(ck, et.double(), rtol=1e-12, atol=0)
    # a different depth moves the bound, not the reference
    ref2, e2, _ = GB.cfg_rescale_axpby(x, eu, et, coef, gs, gr, depth=4096)
    assert torch.equal(ref, ref2) and (e2 >= e).all() and (e2 > e).any()


def test_tree_sum_is_a_sum_and_the_cases_are_the_issues():
    g = torch.Generator().manual_seed(1)
    for n in (2, 252, 4093, GB.RESIDENT + 4):
        v = torch.randn(3, n, generator=g)
        assert torch.allclose(tree_sum(v).double(), v.double().sum(1), rtol=0, atol=GB.chain(n) * RB.U32 * float(v.abs().sum(1).max()))
    shapes = {(s["batch"], s["n"]) for s in GB.CASES.values()}
    assert {(1, 252), (3, 4092), (2, 4096), (2, GB.RESIDENT + 4), (2, 4092), (8, 65536)} <= shapes
    assert GB.RESIDENT == 32768 and GB.CASES[OFFSET]["kind"] == "offset"
