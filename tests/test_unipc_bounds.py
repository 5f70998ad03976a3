"""The bound of tests/unipc_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_unipc.py emulate) stays under the bound on every case
the GPU test runs, over out, last and every history plane; two deliberately wrong restatements land above it -- the coefficient
applied before the difference on rows with a large C2 and a large D1, and 0 * NaN instead of the skipped reads. Ratios are printed
(pytest -s)."""
import pytest
import torch

from tests import unipc_bounds as UB
from tests.abi_emulator_unipc import emulate


def _args(v):
    return v["x"], v["eu"], v["et"], v["last"], v["hist"], v["coef"], v["gs"], v["gr"], v["order"]


@pytest.mark.parametrize("name", list(UB.CASES))
def test_emulation_inside_the_bound(name):
    v = UB.inputs(name)
    ro, rl, rm, off = UB.ratios(v, *emulate(*_args(v)))
    print(f"{name:<44} err/bound: out {ro:.3f}  last {rl:.3f}  plane 0 {rm:.3f}; shifted planes off by {off} elements")
    assert ro < 1.0 and rl < 1.0 and rm < 1.0 and off == 0


def test_the_rows_cover_every_order_and_both_corrector_states():
    k = {n: dict(zip(UB.NAMES, r)) for n, r in UB.ROW.items()}
    assert all(k["full3"][n] != 0.0 for n in UB.NAMES)                                          # every term formed
    assert all(k["first"][n] == 0.0 for n in UB.NAMES[2:7] + UB.NAMES[9:])                      # no corrector, no history
    assert k["second"]["corr"] == 1.0 and k["second"]["C2"] == k["second"]["C3"] == k["second"]["D2"] == 0.0 != k["second"]["D1"]
    assert k["full2"]["C3"] == k["full2"]["D2"] == 0.0 and k["full2"]["C2"] != 0.0 != k["full2"]["D1"]
    assert all(k["full1"][n] == 0.0 for n in ("C2", "C3", "D1", "D2")) and k["full1"]["corr"] == 1.0 != k["full1"]["Ct"]
    assert k["nocorr"]["corr"] == 0.0 and all(k["nocorr"][n] == 0.0 for n in UB.NAMES[2:7]) and k["nocorr"]["D1"] != 0.0
    shapes = {(s["batch"], s["n"], s["order"]) for s in UB.CASES.values()}
    assert {(2, 256, 3), (2, 255, 3), (2, 255, 1), (2, 256, 2), (2, 256, 1), (1, UB.RESIDENT, 3), (1, UB.RESIDENT + 4, 3)} <= shapes


def _close_planes(name, **scaled):
    """the case's inputs on the full third-order row with the named coefficients at 400 times Bc / Bp and every plane within 1e-4 of
    what it is subtracted from"""
    v = UB.inputs(name)
    row = dict(zip(UB.NAMES, UB.FULL3))
    for n, base in scaled.items():
        row[n] = 400.0 * row[base]
    v["coef"] = torch.tensor([row[n] for n in UB.NAMES], dtype=torch.float32)
    mt = UB.unipc_update(*_args(v))["mt"]
    g = torch.Generator().manual_seed(3)
    v["hist"][0] = (mt * (1 + 1e-4 * torch.randn(mt.shape, generator=g, dtype=torch.float64))).float()
    for j in (1, 2):
        v["hist"][j] = (v["hist"][0].double() * (1 + 1e-4 * torch.randn(mt.shape, generator=g, dtype=torch.float64))).float()
    return v


def test_coefficient_before_the_difference_is_outside_the_bound():
    """C_k and D_k carry 1 / r_k. On a row with C2 = 400 Bc and planes close to each other, C2 h2 - C2 h1 rounds at |C2| (|h2| + |h1|)
    where the reference form rounds at |C2| |h2 - h1|: last leaves the bound, and out = Ap x_c + ... with it. The planes are read, not
    computed, so nothing in the bound hides it. The reference form on the same row stays inside."""
    v = _close_planes("b2 n256 o3 vectors", C2="Bc")
    go, gl, gm, _ = UB.ratios(v, *emulate(*_args(v)))
    bo, bl, bm, _ = UB.ratios(v, *emulate(*_args(v), fault="regroup"))
    print(f"C2 = 400 Bc, close planes: reference form out {go:.3f} last {gl:.3f}; regrouped out {bo:.3g} last {bl:.3g}")
    assert go < 1.0 and gl < 1.0 and gm < 1.0 and bo > 1.0 and bl > 1.0


def test_regrouped_predictor_difference_is_outside_the_bound():
    """The predictor's differences are against the COMPUTED m_t: the bound already holds |D1| e_mt >= 2 u |D1| |m_t| for it, so the
    regrouped D1 h1 - D1 m_t cannot land far outside (as tests/test_multistep_bounds.py notes of its D). Without guidance e_mt is
    smallest, and D1 = 400 Bp leaves the bound; the reference form stays inside."""
    v = _close_planes("b2 n256 o3 no eps_text", D1="Bp")
    good = UB.ratios(v, *emulate(*_args(v)))
    bad = UB.ratios(v, *emulate(*_args(v), fault="regroup"))
    print(f"D1 = 400 Bp, h1 = m_t (1 + 1e-4 N): reference form out {good[0]:.3f}, regrouped out {bad[0]:.3g}")
    assert max(good[:3]) < 1.0 < bad[0]


@pytest.mark.parametrize("name", ["b2 n256 o3 first step NaN state", "b2 n256 o3 second step NaN planes 1 2"])
def test_zero_times_nan_is_outside_the_bound(name):
    v = UB.inputs(name)
    good = UB.ratios(v, *emulate(*_args(v)))
    bad = UB.ratios(v, *emulate(*_args(v), fault="mul_nan"))
    print(f"{name}: skipped reads {good}, 0 * NaN {bad}")
    assert max(good[:3]) < 1.0 and good[3] == 0 and bad[0] == float("inf")
