"""The bound of tests/dpm2_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_dpm2.py emulate) stays under the bound on every case
the GPU test runs -- out, and the parked sample bit for bit; deliberately wrong restatements land far above it: stage 2 starting from
x instead of the parked sample, c z formed at c = 0 over a NaN plane, stage 1 reading a NaN S, and the noise rounded to bfloat16 before
use. Ratios are printed (pytest -s)."""
import pytest
import torch

from tests import dpm2_bounds as DB
from tests.abi_emulator_dpm2 import emulate

FAR = 100.0   # "far above": two orders over the bound


def _run(v, fault=None):
    return DB.ratios(v, *emulate(v["x"], v["eu"], v["et"], v["z"], v["S"], v["coef"], v["gs"], v["gr"], fault=fault))


@pytest.mark.parametrize("name", list(DB.CASES))
def test_emulation_inside_the_bound(name):
    r = _run(DB.inputs(name))
    print(f"{name:<52} out err/bound {r['out']:.3f}  S elements off {r['S_off']}")
    assert r["out"] < 1.0 and r["S_off"] == 0


def test_the_cases_cover_every_form_row_and_stage():
    R = DB.ROW
    assert R["v1"][0] != 0.0 and R["v1"][3:] == (0.0, 0.0) and R["v2"][0] != 0.0 and R["v2"][3] > 0.0 and R["v2"][4] == 1.0
    assert R["eps1"][:2] == (0.0, 1.0) and R["eps1"][3:] == (0.0, 0.0) and R["eps2"][:2] == (0.0, 1.0) and R["eps2"][3] > 0.0
    assert R["last"][3:] == (0.0, 0.0) and R["v2c0"][0] != 0.0 and R["v2c0"][3:] == (0.0, 1.0) and R["eps2c0"][:2] == (0.0, 1.0)
    assert R["eps2c0"][3:] == (0.0, 1.0)
    for rows in (DB.ROWS_V, DB.ROWS_EPS, DB.ROWS_V0, DB.ROWS_EPS0):   # even: stage 1, odd: stage 2, the last: stage 1
        assert len(rows) == 39 and all(r[4] == i % 2 for i, r in enumerate(rows)) and all(r[2] < 0.0 for r in rows)
    assert all(r[3] == 0.0 for r in DB.ROWS_V0 + DB.ROWS_EPS0) and all((r[3] > 0.0) == (r[4] == 1.0) for r in DB.ROWS_V + DB.ROWS_EPS)
    shapes = {(s["batch"], s["n"], s.get("gr", 0.0) > 0, R[s["row"]][4]) for s in DB.CASES.values()}
    for second in (0.0, 1.0):
        assert {(2, 512, False, second), (1, 251, False, second), (1, 252, False, second), (1, 1, False, second), (2, 1024, True, second),
                (1, 2, True, second), (3, 1023, True, second), (2, DB.RESIDENT, True, second), (2, DB.RESIDENT + 4, True, second)} <= shapes
        assert {s.get("misalign") for s in DB.CASES.values() if R[s["row"]][4] == second} == {None, *DB.POINTERS}
        assert any(s.get("alias") and R[s["row"]][4] == second for s in DB.CASES.values())
        assert any(not s.get("cfg", True) and R[s["row"]][4] == second for s in DB.CASES.values())
    for gr in (0.0, 0.7):   # every read a row must not make, over NaN, in both kernel forms
        of = [s for s in DB.CASES.values() if s.get("gr", 0.0) == gr]
        assert any(s.get("nan") == ("S", "z") and R[s["row"]][4] == 0.0 for s in of)
        assert any(s.get("nan") == ("z",) and R[s["row"]][3:] == (0.0, 1.0) and not s.get("null_noise") for s in of)
        assert any(s.get("nan") == ("z",) and R[s["row"]][3:] == (0.0, 1.0) and s.get("null_noise") for s in of)
        assert any(s.get("nan") == ("x",) and R[s["row"]][0] == 0.0 and R[s["row"]][4] == 1.0 for s in of)
    assert all(R[s["row"]][4] == 0.0 or R[s["row"]][3] == 0.0 for s in DB.CASES.values() if s.get("null_noise"))
    assert any(s.get("kind") == "offset" for s in DB.CASES.values())


@pytest.mark.parametrize("name", ["b2 n512 vectors stage 2", "b2 n512 epsilon row stage 2", "b2 n512 stage 2 c0", "b2 n1024 rescale stage 2"])
def test_stage_two_from_x_instead_of_the_parked_sample_is_outside_the_bound(name):
    v = DB.inputs(name)
    good, bad = _run(v), _run(v, fault="from_x")
    print(f"{name}: from S {good['out']:.3f}, from x {bad['out']:.3g}")
    assert good["out"] < 1.0 and bad["out"] > FAR


@pytest.mark.parametrize("name", ["b2 n512 stage 2 c0 NaN noise", "b1 n251 stage 2 c0 NaN noise", "b2 n1024 rescale stage 2 c0 NaN noise"])
def test_c_times_z_formed_at_c_zero_over_a_nan_plane_is_outside_the_bound(name):
    v = DB.inputs(name)
    good, bad = _run(v), _run(v, fault="mul_nan")
    print(f"{name}: skipped read {good['out']:.3f}, 0 * NaN {bad['out']}")
    assert good["out"] < 1.0 and good["S_off"] == 0 and bad["out"] == float("inf")


@pytest.mark.parametrize("name", ["b2 n512 stage 1 NaN S and noise", "b1 n251 stage 1 NaN S and noise",
                                  "b2 n1024 rescale stage 1 NaN S and noise"])
def test_stage_one_reading_a_nan_sample_is_outside_the_bound(name):
    v = DB.inputs(name)
    good, bad = _run(v), _run(v, fault="mul_nan")
    print(f"{name}: skipped read {good['out']:.3f}, 0 * NaN {bad['out']}")
    assert good["out"] < 1.0 and good["S_off"] == 0 and bad["out"] == float("inf")


@pytest.mark.parametrize("name", ["b2 n512 vectors stage 2", "b2 n512 epsilon row stage 2", "b2 n1024 rescale stage 2"])
def test_noise_rounded_to_bf16_is_outside_the_bound(name):
    """z is read, not computed: the bound holds 2 u |c z| for it (plus its share of 2 u |ref|), a bfloat16 plane is off by up to
    2^-9 |c z|"""
    v = DB.inputs(name)
    good, bad = _run(v), _run(v, fault="bf16_noise")
    print(f"{name}: fp32 noise {good['out']:.3f}, bf16 noise {bad['out']:.3g}")
    assert good["out"] < 1.0 and bad["out"] > FAR


def test_a_parked_sample_that_is_not_a_bit_copy_is_counted():
    v = DB.inputs("b2 n512 vectors stage 1")
    out, S = emulate(v["x"], v["eu"], v["et"], v["z"], v["S"], v["coef"], v["gs"], v["gr"])
    S = S.clone()
    S[1, 7] = torch.nextafter(S[1, 7], torch.tensor(float("inf")))
    assert DB.ratios(v, out, S)["S_off"] == 1


def test_accumulated_carries_the_parked_sample_through_both_stages():
    """two launches (one DPM2 a step) by hand: the bound after stage 2 starts from the error of the PARKED sample, not from the latents'
    after stage 1"""
    g = torch.Generator().manual_seed(3)
    x0, o1, o2, z = (torch.randn(2, 4, 4, 4, generator=g) for _ in range(4))
    rows = DB.ROWS_V[10:12]
    c = [torch.tensor(r, dtype=torch.float32) for r in rows]
    f = lambda t: t.flatten(1)  # noqa: E731
    x1, S = emulate(f(x0), f(o1), None, None, f(x0), c[0], 1.0, 0.0)
    x2, _ = emulate(x1, f(o2), None, f(z), S, c[1], 1.0, 0.0)
    E = DB.accumulated([x0, x1.reshape(x0.shape)], [x0, S.reshape(x0.shape)], [None, z], [o1, o2], rows, 1.0, 0.0, cfg=False)
    p, q, h, _, _ = rows[0]
    y1 = x0.double() + h * (p * x0.double() + q * o1.double())
    p2, q2, h2, c2, _ = rows[1]
    want = x0.double() + h2 * (p2 * y1 + q2 * o2.double()) + c2 * z.double()
    r1 = ((x1.reshape(x0.shape).double() - y1).abs() / E[0]).max().item()
    r2 = ((x2.reshape(x0.shape).double() - want).abs() / E[1]).max().item()
    print(f"by hand: after stage 1 {r1:.3f}, after stage 2 {r2:.3f} of the accumulated bound")
    assert r1 < 1.0 and r2 < 1.0 and (E[1] > 0).all()
