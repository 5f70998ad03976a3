"""The bound of tests/ancestral_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_ancestral.py emulate) stays under the bound on every
case the GPU test runs; three deliberately wrong restatements land above it -- c * z formed at c = 0 over a NaN plane, the noise
rounded to bfloat16 before use, and the one-pass fp32 variance in the rescale form. Ratios are printed (pytest -s)."""
import pytest

from tests import ancestral_bounds as AB
from tests.abi_emulator_ancestral import emulate


def _args(v, null=False):
    return v["x"], v["eu"], v["et"], None if null else v["z"], v["coef"], v["gs"], v["gr"]


@pytest.mark.parametrize("name", list(AB.CASES))
def test_emulation_inside_the_bound(name):
    v = AB.inputs(name)
    r = AB.ratio(v, emulate(*_args(v, AB.CASES[name].get("null_noise", False))))
    print(f"{name:<44} err/bound {r:.3f}")
    assert r < 1.0


def test_the_cases_cover_every_form_and_row():
    a, b, c = AB.ROW["mid"]
    assert a != 1.0 and b != 0.0 and c != 0.0
    assert AB.ROW["eps"][0] == 1.0 and AB.ROW["eps"][2] != 0.0
    assert AB.ROW["last"][2] == 0.0 and AB.ROW["last"][1] != 0.0
    shapes = {(s["batch"], s["n"], s.get("gr", 0.0) > 0) for s in AB.CASES.values()}
    assert {(2, 512, False), (1, 252, False), (1, 251, False), (2, 1024, True), (2, AB.RESIDENT, True), (2, AB.RESIDENT + 4, True)} <= shapes
    assert {s.get("misalign") for s in AB.CASES.values()} == {None, *AB.POINTERS}   # each pointer in turn, noise included
    for gr in (0.0, 0.7):   # c == 0 over NaN noise and over a null plane, in both kernel forms
        assert any(s.get("nan_noise") and not s.get("null_noise") and s.get("gr", 0.0) == gr for s in AB.CASES.values())
        assert any(s.get("null_noise") and s.get("gr", 0.0) == gr for s in AB.CASES.values())


@pytest.mark.parametrize("name", ["b2 n512 c0 NaN noise", "b2 n1024 rescale c0 NaN noise"])
def test_zero_times_nan_is_outside_the_bound(name):
    v = AB.inputs(name)
    good = AB.ratio(v, emulate(*_args(v)))
    bad = AB.ratio(v, emulate(*_args(v), fault="mul_nan"))
    print(f"{name}: skipped read {good:.3f}, 0 * NaN {bad}")
    assert good < 1.0 and bad == float("inf")


@pytest.mark.parametrize("name", ["b2 n512 vectors", "b2 n512 epsilon row", "b2 n1024 rescale"])
def test_noise_rounded_to_bf16_is_outside_the_bound(name):
    """z is read, not computed: the bound holds 2 u |c z| for it (plus its share of 2 u |ref|), a bfloat16 plane is off by up to
    2^-9 |c z|"""
    v = AB.inputs(name)
    good = AB.ratio(v, emulate(*_args(v)))
    bad = AB.ratio(v, emulate(*_args(v), fault="bf16_noise"))
    print(f"{name}: fp32 noise {good:.3f}, bf16 noise {bad:.3g}")
    assert good < 1.0 < bad


def test_one_pass_variance_is_outside_the_bound():
    v = AB.inputs("b2 n1024 rescale offset 64")
    good = AB.ratio(v, emulate(*_args(v)))
    bad = AB.ratio(v, emulate(*_args(v), fault="one_pass"))
    print(f"offset case: two-pass {good:.3f}, one-pass fp32 variance {bad:.3g}")
    assert good < 1.0 < bad
