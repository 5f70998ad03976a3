"""The bound of tests/heun_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_heun.py emulate) stays under the bound on every case
the GPU test runs -- out, the stage-1 derivative, and the parked sample bit for bit; deliberately wrong restatements land above it:
stage 2 starting from x instead of the parked sample, the terms over state a stage must not read formed with a zero weight over NaN
planes (stage 1, and stage 2 at g == 0), and the parked derivative rounded to bfloat16 before use. Ratios are printed (pytest -s)."""
import pytest
import torch

from tests import heun_bounds as HB
from tests.abi_emulator_heun import emulate


def _run(v, fault=None):
    return HB.ratios(v, *emulate(v["x"], v["eu"], v["et"], v["S"], v["D"], v["coef"], v["gs"], v["gr"], fault=fault))


@pytest.mark.parametrize("name", list(HB.CASES))
def test_emulation_inside_the_bound(name):
    r = _run(HB.inputs(name))
    print(f"{name:<48} out err/bound {r['out']:.3f}  D {r['D']:.3f}  S / D elements off {r['S_off']}")
    assert r["out"] < 1.0 and r["D"] < 1.0 and r["S_off"] == 0


def test_the_cases_cover_every_form_row_and_stage():
    R = HB.ROW
    assert R["v1"][0] != 0.0 and R["v1"][3:] == (0.0, 0.0) and R["v2"][0] != 0.0 and R["v2"][3:] == (1.0, 1.0)
    assert R["eps1"][:2] == (0.0, 1.0) and R["eps1"][4] == 0.0 and R["eps2"][:2] == (0.0, 1.0) and R["eps2"][4] == 1.0
    assert R["last"][4] == 0.0 and R["g0"][3:] == (0.0, 1.0) and R["g0"][:3] == R["v2"][:3]
    assert len(HB.ROWS_V) == 39 and all(r[4] == i % 2 for i, r in enumerate(HB.ROWS_V))   # even: stage 1, odd: stage 2, the last: stage 1
    assert R["v2"][2] == R["v1"][2] / 2                                                    # h of stage 2 is half the parked dt
    shapes = {(s["batch"], s["n"], s.get("gr", 0.0) > 0, R[s["row"]][4]) for s in HB.CASES.values()}
    for second in (0.0, 1.0):
        assert {(2, 512, False, second), (1, 251, False, second), (1, 252, False, second), (1, 1, False, second), (2, 1024, True, second),
                (1, 2, True, second), (3, 1023, True, second), (2, HB.RESIDENT, True, second), (2, HB.RESIDENT + 4, True, second)} <= shapes
        assert {s.get("misalign") for s in HB.CASES.values() if R[s["row"]][4] == second} == {None, *HB.POINTERS}
        assert any(s.get("alias") and R[s["row"]][4] == second for s in HB.CASES.values())
        assert any(not s.get("cfg", True) and R[s["row"]][4] == second for s in HB.CASES.values())
    for gr in (0.0, 0.7):   # stage 1 over NaN S and D, stage 2 at g == 0 over a NaN D, in both kernel forms
        assert any(s.get("nan") == ("S", "D") and s.get("gr", 0.0) == gr for s in HB.CASES.values())
        assert any(s.get("nan") == ("D",) and s["row"] == "g0" and s.get("gr", 0.0) == gr for s in HB.CASES.values())
    assert any(s.get("kind") == "offset" for s in HB.CASES.values())


@pytest.mark.parametrize("name", ["b2 n512 vectors stage 2", "b2 n512 epsilon row stage 2", "b2 n1024 rescale stage 2"])
def test_stage_two_from_x_instead_of_the_parked_sample_is_outside_the_bound(name):
    v = HB.inputs(name)
    good, bad = _run(v), _run(v, fault="from_x")
    print(f"{name}: from S {good['out']:.3f}, from x {bad['out']:.3g}")
    assert good["out"] < 1.0 < bad["out"]


@pytest.mark.parametrize("name", ["b2 n512 stage 1 NaN state", "b2 n1024 rescale stage 1 NaN state", "b2 n512 stage 2 g0 NaN D",
                                  "b2 n1024 rescale stage 2 g0 NaN D"])
def test_zero_times_nan_state_is_outside_the_bound(name):
    v = HB.inputs(name)
    good, bad = _run(v), _run(v, fault="mul_nan")
    print(f"{name}: skipped read {good['out']:.3f}, 0 * NaN {bad['out']}")
    assert good["out"] < 1.0 and good["D"] < 1.0 and good["S_off"] == 0 and bad["out"] == float("inf")


@pytest.mark.parametrize("name", ["b2 n512 vectors stage 2", "b2 n512 epsilon row stage 2", "b2 n1024 rescale stage 2"])
def test_derivative_rounded_to_bf16_is_outside_the_bound(name):
    """D is read, not computed: the bound holds u |h D| for it (plus its share of 2 u |ref|), a bfloat16 plane is off by up to
    2^-9 |h D|"""
    v = HB.inputs(name)
    good, bad = _run(v), _run(v, fault="bf16_deriv")
    print(f"{name}: fp32 derivative {good['out']:.3f}, bf16 derivative {bad['out']:.3g}")
    assert good["out"] < 1.0 < bad["out"]


def test_a_parked_sample_that_is_not_a_bit_copy_is_counted():
    v = HB.inputs("b2 n512 vectors stage 1")
    out, S, D = emulate(v["x"], v["eu"], v["et"], v["S"], v["D"], v["coef"], v["gs"], v["gr"])
    S = S.clone()
    S[1, 7] = torch.nextafter(S[1, 7], torch.tensor(float("inf")))
    assert HB.ratios(v, out, S, D)["S_off"] == 1


def test_accumulated_carries_the_state_through_both_stages():
    """two launches (one Heun step) by hand: the bound after stage 2 starts from the error of the PARKED sample, not from the latents'
    after stage 1, and takes the parked derivative's error through |h| g"""
    g = torch.Generator().manual_seed(3)
    x0, o1, o2 = (torch.randn(2, 4, 4, 4, generator=g) for _ in range(3))
    rows = HB.ROWS_V[10:12]
    c = [torch.tensor(r, dtype=torch.float32) for r in rows]
    f = lambda t: t.flatten(1)  # noqa: E731
    x1, S, D = emulate(f(x0), f(o1), None, f(x0), f(x0), c[0], 1.0, 0.0)
    x2, _, _ = emulate(x1, f(o2), None, S, D, c[1], 1.0, 0.0)
    E = HB.accumulated([x0, x1.reshape(x0.shape)], [(x0, x0), (S.reshape(x0.shape), D.reshape(x0.shape))], [o1, o2], rows, 1.0, 0.0,
                       cfg=False)
    p, q, h, _, _ = rows[0]
    d1 = p * x0.double() + q * o1.double()
    y1 = x0.double() + h * d1
    p2, q2, h2, _, _ = rows[1]
    want = x0.double() + h2 * (d1 + p2 * y1 + q2 * o2.double())
    r1 = ((x1.reshape(x0.shape).double() - y1).abs() / E[0]).max().item()
    r2 = ((x2.reshape(x0.shape).double() - want).abs() / E[1]).max().item()
    print(f"by hand: after stage 1 {r1:.3f}, after stage 2 {r2:.3f} of the accumulated bound")
    assert r1 < 1.0 and r2 < 1.0 and (E[1] > 0).all()
