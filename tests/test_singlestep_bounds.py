"""The bound of tests/singlestep_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_singlestep.py emulate) stays under the bound on every
case the GPU test runs -- out, the written plane, and every bit of the state a row must leave alone; deliberately wrong restatements
land outside it: the regrouped (cancelling) sum, an order-1 row that reads the parked sample, an order-2 row that parks, an order-2 row
that skips the plane-1 store, and a zero-weighted term formed over NaN state. Ratios are printed (pytest -s)."""
import pytest
import torch

from tests import singlestep_bounds as SB
from tests.abi_emulator_singlestep import emulate
from tests.step_forms import FORMS
from tests.test_step_forms import _check


def _run(v, fault=None):
    return SB.ratios(v, *emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"], fault=fault))


def _good(r):
    return r["out"] < 1.0 and r["hist"] < 1.0 and r["state_off"] == 0


def test_the_form_row_agrees_with_its_signature():
    form = FORMS["singlestep"]
    _check(form)
    assert form.entry == "singlestep_update" and form.width == SB.WIDTH == 8


@pytest.mark.parametrize("name", list(SB.CASES))
def test_emulation_inside_the_bound(name):
    r = _run(SB.inputs(name))
    print(f"{name:<52} out err/bound {r['out']:.3f}  written plane {r['hist']:.3f}  state elements off {r['state_off']}")
    assert _good(r)


def test_the_cases_cover_every_form_row_and_state():
    R, C = SB.ROW, SB.CASES.values()
    for k in ("v", "eps"):
        assert [SB.flags(R[f"{k}_{kind}"]) for kind in SB.KINDS] == [(1, False, False), (2, True, False), (3, False, True),
                                                                     (3, False, False), (2, False, False)]
        assert R[f"{k}_o3h"][5] != 0.0 and R[f"{k}_o3m"][5] == 0.0 and R[f"{k}_o1"][4:6] == (0.0, 0.0)
        assert all(R[f"{k}_{kind}"][4] != 0.0 for kind in SB.KINDS[1:])
    assert all(R[f"v_{kind}"][0] != 0.0 for kind in SB.KINDS) and all(R[f"eps_{kind}"][:2] == (0.0, 1.0) for kind in SB.KINDS)
    assert all(len(r) == SB.WIDTH for r in R.values())
    shapes = {(s["batch"], s["n"], s.get("gr", 0.0) > 0, s["row"]) for s in C}
    for r in R:   # every kind of row, both prediction types, on every kernel path
        assert {(2, 512, False, r), (1, 251, False, r), (3, 1023, False, r), (2, 1024, True, r), (2, SB.RESIDENT + 4, True, r)} <= shapes
    for r in ("v_o1", "v_o2k1", "v_o3h"):
        assert {s.get("misalign") for s in C if s["row"] == r} == {None, *SB.POINTERS}
        assert any(s.get("alias") and s["row"] == r for s in C) and any(not s.get("cfg", True) and s["row"] == r for s in C)
    assert 251 % 4 and (3 * 1023) % 4   # planes that are not 16-byte aligned: the vector path is refused
    # every case holds NaN in whatever its row must not read
    for name, s in SB.CASES.items():
        v = SB.inputs(name)
        order, keep, heun = SB.flags(v["coef"])
        assert torch.isnan(v["P"]).all() == (order == 1) and torch.isnan(v["H"][0]).all() == (order == 1), name
        assert torch.isnan(v["H"][1]).all() == (not heun), name
        assert torch.isfinite(v["x"]).all()


FAULTS = {   # fault: the cases it must show on (a row that forms the term in question), and where it shows
    "read_park_o1": (["b2 n512 vectors v_o1", "b1 n251 scalar, unaligned planes eps_o1", "b2 n1024 rescale v_o1"], "out"),
    "park_o2": (["b2 n512 vectors v_o2k1", "b2 n512 vectors eps_o2k0", "b2 n1024 rescale v_o2k0"], "state_off"),
    "skip_keep": (["b2 n512 vectors v_o2k1", "b3 n1023 scalar, odd eps_o2k1", "b2 n1024 rescale v_o2k1"], "hist"),
    "mul_nan": (["b2 n512 vectors v_o2k1", "b2 n512 vectors eps_o3m", "b2 n1024 rescale v_o2k0", "b2 n1024 rescale v_o3m"], "out"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_an_injected_fault_is_outside_the_bound(fault):
    names, where = FAULTS[fault]
    for name in names:
        v = SB.inputs(name)
        good, bad = _run(v), _run(v, fault=fault)
        print(f"{fault} on {name}: right {good[where]:.3g}, faulty {bad[where]:.3g}")
        assert _good(good)
        assert bad[where] > (0 if where == "state_off" else 1.0)


@pytest.mark.parametrize("row", ["eps_o2k1", "eps_o3h", "eps_o3m"])
def test_regrouped_differences_are_outside_the_bound(row):
    """E1 and E2 carry the reciprocals of the step ratios: on a row with E1 = 400 B (and E2 = -300 B where the row has one) and a
    group whose outputs are within 1e-4 of m0, the regrouped sum rounds at |E1| |m0| where the reference form rounds at
    |E1| |m0 - b|. The reference form on the same row stays inside. Rows with p = 0, q = 1 and no guidance: m0 is then the model
    output itself. (Where m0 is computed the bound already holds |E1| e_m0 >= 2 u |E1| |m0| for its entering the difference, and
    the regrouped form cannot land far outside, as tests/test_multistep_bounds.py notes for its own.)"""
    v = SB.inputs(f"b2 n512 no eps_text {row}")
    c = list(SB.ROW[row])
    c[4], c[5] = 400.0 * c[3], (-300.0 * c[3] if c[5] != 0.0 else 0.0)
    v["coef"] = torch.tensor(c, dtype=torch.float32)
    m0 = SB.singlestep_update(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"])["m0"]
    near = 1e-4 * torch.randn((2,) + tuple(m0.shape), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    H = (m0 * (1 + near)).float()
    H[1] = torch.where(torch.isnan(v["H"][1]), v["H"][1], H[1])   # (NaN stays where the row does not read)
    v["H"] = H
    good, bad = _run(v), _run(v, fault="regroup")
    print(f"{row}: E1 = 400 B, the group within 1e-4 of m0: reference form {good['out']:.3f}, regrouped form {bad['out']:.3g}")
    assert _good(good) and bad["out"] > 1.0


def test_state_that_is_not_what_it_must_be_is_counted():
    v = SB.inputs("b2 n512 vectors v_o2k1")
    out, P, H = emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"])
    assert SB.ratios(v, out, P, H)["state_off"] == 0
    P2 = P.clone()
    P2[1, 7] = torch.nextafter(P2[1, 7], torch.tensor(float("inf")))
    H2 = H.clone()
    H2[0, 0, 3] += 1.0   # the plane an order-2 row does not write
    assert SB.ratios(v, out, P2, H)["state_off"] == 1 and SB.ratios(v, out, P, H2)["state_off"] == 1


@pytest.mark.parametrize("solver", ["heun", "midpoint"])
def test_accumulated_carries_the_planes_and_the_parked_sample(solver):
    """seven launches by hand (orders 1 2 3 1 2 3 1): float64 with the float64 rows against the restatement with the fp32 table, to
    the accumulated bound after every launch"""
    g = torch.Generator().manual_seed(3)
    shape = (2, 4, 4, 4)
    x0 = torch.randn(shape, generator=g)
    rows = SB.schedule_rows(prediction_type="v_prediction", solver_order=3, solver_type=solver)[6:13]
    assert [int(r[6]) for r in rows] == [1, 2, 3, 1, 2, 3, 1]
    outs = [torch.randn(shape, generator=g) for _ in rows]
    f = lambda t: t.flatten(1)  # noqa: E731
    x, P, H = f(x0), torch.full_like(f(x0), float("nan")), torch.full((2,) + tuple(f(x0).shape), float("nan"))
    xs, states, ends = [], [], []
    for o, row in zip(outs, rows):
        xs.append(x.reshape(shape))
        states.append((P.reshape(shape), H.reshape((2,) + shape)))
        x, P, H = emulate(x, f(o), None, P, H, torch.tensor(row, dtype=torch.float32), 1.0, 0.0)
        ends.append(x.reshape(shape))
    E = SB.accumulated(xs, states, outs, rows, 1.0, 0.0, cfg=False)
    y = x0.double()
    for i, (o, row) in enumerate(zip(outs, rows)):
        p, q, A, B, E1, E2, order, keep = row
        m0 = p * y + q * o.double()
        if order == 1.0:
            S, base, y = y, m0, A * y + B * m0
        else:
            y = A * S + B * base + E1 * (m0 - base) + (E2 * (m1 - base) if order == 3.0 and E2 != 0.0 else 0.0)
            if keep:
                m1 = m0
        ratio = ((ends[i].double() - y).abs() / E[i]).max().item()
        print(f"{solver} by hand: after launch {i} (order {int(order)}) {ratio:.3f} of the accumulated bound")
        assert ratio < 1.0 and (E[i] > 0).all()
