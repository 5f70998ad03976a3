"""The bound of tests/plms_bounds.py, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_plms.py emulate) stays under the bound on every case the
GPU test runs -- out, the written ring plane, and every bit of the state a row must leave alone; deliberately wrong restatements land
outside it: two ring planes exchanged, the averaging row started from x, e stored on the averaging row, the conversion taken with x,
the fourth term dropped, e stored after its conversion, and zero-weighted terms formed over NaN state. Ratios are printed (pytest -s)."""
import pytest
import torch

from tests import plms_bounds as PB
from tests.abi_emulator_plms import emulate


def _run(v, fault=None):
    return PB.ratios(v, *emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"], fault=fault))


def _good(r):
    return r["out"] < 1.0 and r["hist"] < 1.0 and r["state_off"] == 0


@pytest.mark.parametrize("name", list(PB.CASES))
def test_emulation_inside_the_bound(name):
    r = _run(PB.inputs(name))
    print(f"{name:<52} out err/bound {r['out']:.3f}  written plane {r['hist']:.3f}  state elements off {r['state_off']}")
    assert _good(r)


def test_the_cases_cover_every_form_row_and_state():
    R, C = PB.ROW, PB.CASES.values()
    for k in ("v", "eps"):
        assert [R[f"{k}{c}"][8:11] for c in range(7)] == [(0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, 0.0),
                                                          (1.0, 0.0, 0.0), (2.0, 0.0, 0.0)]
        assert [sum(w != 0.0 for w in R[f"{k}{c}"][4:8]) for c in range(5)] == [1, 2, 2, 3, 4]
    assert all(R[f"v{c}"][2] != 0.0 for c in range(7)) and all(R[f"eps{c}"][2:4] == (0.0, 1.0) for c in range(7))
    assert len(PB.ROWS_V) == 21 and R["last"] == PB.ROWS_V[-1] and all(len(r) == PB.WIDTH for r in PB.ROWS_V)
    shapes = {(s["batch"], s["n"], s.get("gr", 0.0) > 0, s["row"]) for s in C}
    for c in range(5):   # every counter, both prediction types, on the vector path; the wrap row (v4 / eps4: slot 0, three live planes)
        assert {(2, 512, False, f"v{c}"), (2, 512, False, f"eps{c}"), (2, 1024, True, f"v{c}")} <= shapes
    for r in ("v0", "v1", "v4"):
        assert {(1, 251, False, r), (1, 1, False, r), (1, 2, True, r), (3, 1023, True, r), (2, PB.RESIDENT + 4, True, r)} <= shapes
        assert {s.get("misalign") for s in C if s["row"] == r} == {None, *PB.POINTERS}
        assert any(s.get("alias") and s["row"] == r for s in C) and any(not s.get("cfg", True) and s["row"] == r for s in C)
    assert (2, PB.RESIDENT, True, "v4") in shapes and any(s.get("kind") == "offset" for s in C)
    assert 251 % 4 and (2 * 251) % 4   # a ring whose planes are not 16-byte aligned: the vector path is refused
    for gr in (0.0, 0.7):   # a row over NaN in everything it must not read, in both kernel forms
        for nan in (("P", "h1", "h2", "h3"), ("x", "h2", "h3"), ("h2", "h3", "P")):
            assert any(s.get("nan") == nan and s.get("gr", 0.0) == gr for s in C)


FAULTS = {   # fault: the cases it must show on (a row that forms the term in question), and where it shows
    "swap_h12": (["b2 n512 vectors v3", "b2 n512 vectors eps4", "b2 n1024 rescale v4", "b2 n512 vectors eps2"], "out"),
    "from_x": (["b2 n512 vectors v1", "b2 n512 vectors eps1", "b2 n1024 rescale v1", "b1 n251 scalar, unaligned planes v1"], "out"),
    "append_avg": (["b2 n512 vectors v1", "b2 n512 vectors eps1", "b2 n1024 rescale v1"], "state_off"),
    "convert_x": (["b2 n512 vectors v1", "b2 n1024 rescale v1", "b1 n251 scalar, unaligned planes v1"], "out"),
    "drop_w3": (["b2 n512 vectors v4", "b2 n512 vectors eps4", "b2 n1024 rescale v4", "b2 n512 vectors v6"], "out"),
    "store_converted": (["b2 n512 vectors v0", "b2 n512 vectors v4", "b2 n1024 rescale v2"], "hist"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_an_injected_fault_is_outside_the_bound(fault):
    names, where = FAULTS[fault]
    for name in names:
        v = PB.inputs(name)
        good, bad = _run(v), _run(v, fault=fault)
        print(f"{fault} on {name}: right {good[where]:.3g}, faulty {bad[where]:.3g}")
        assert _good(good)
        assert bad[where] > (0 if where == "state_off" else 1.0)


@pytest.mark.parametrize("name", [n for n, s in PB.CASES.items() if s.get("nan")])
def test_zero_times_nan_state_is_outside_the_bound(name):
    v = PB.inputs(name)
    good, bad = _run(v), _run(v, fault="mul_nan")
    print(f"{name}: skipped read {good['out']:.3f}, 0 * NaN {bad['out']}")
    assert _good(good) and bad["out"] == float("inf")


def test_the_absolute_sum_of_the_four_term_row_is_carried():
    """a smooth history: h1 = h2 = h3 = E, so the terms cancel from an absolute sum of 160 / 24 |E| to m = E. The roundings happen on
    the terms, not on m: the bound must allow 160 / 24 times what the size of m suggests, and the restatement must still be inside"""
    v = PB.inputs("b2 n512 no eps_text eps3")
    v["coef"] = torch.tensor(PB.ROW["eps4"], dtype=torch.float32)
    v["H"] = v["eu"].expand(3, -1, -1).clone()
    r = PB.plms_update(v["x"], v["eu"], None, v["P"], v["H"], v["coef"], 1.0, 0.0)
    out, _, _ = emulate(v["x"], v["eu"], None, v["P"], v["H"], v["coef"], 1.0, 0.0)
    bound = 2 * PB.U32 * r["out"].abs() + r["e_out"]
    share = r["e_out"] / (abs(float(v["coef"][1])) * PB.U32 * r["m"].abs())   # the bound in roundings of b m
    print(f"smooth history: err / bound {float(((out.double() - r['out']).abs() / bound).max()):.3f}, "
          f"e_out is at least {float(share.min()):.1f} roundings of |b m|")
    assert ((out.double() - r["out"]).abs() <= bound).all()
    assert torch.allclose(r["m"], v["eu"].double(), rtol=1e-6, atol=0) and float(share.min()) > 4 * 160 / 24   # K = 4 roundings per term


def test_state_that_is_not_what_it_must_be_is_counted():
    v = PB.inputs("b2 n512 vectors v0")
    out, P, H = emulate(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"])
    assert PB.ratios(v, out, P, H)["state_off"] == 0
    P2 = P.clone()
    P2[1, 7] = torch.nextafter(P2[1, 7], torch.tensor(float("inf")))
    H2 = H.clone()
    H2[2, 0, 3] += 1.0   # a plane the row does not write
    assert PB.ratios(v, out, P2, H)["state_off"] == 1 and PB.ratios(v, out, P, H2)["state_off"] == 1


def test_accumulated_carries_the_ring_and_the_parked_sample():
    """five launches by hand (counter 0 .. 4, the last one the wrap): float64 with the float64 rows against the restatement with the
    fp32 table, to the accumulated bound after every launch"""
    g = torch.Generator().manual_seed(3)
    shape = (2, 4, 4, 4)
    x0 = torch.randn(shape, generator=g)
    outs = [torch.randn(shape, generator=g) for _ in range(5)]
    rows = PB.ROWS_V[:5]
    f = lambda t: t.flatten(1)  # noqa: E731
    x, P, H = f(x0), torch.full_like(f(x0), float("nan")), torch.full((3,) + tuple(f(x0).shape), float("nan"))
    xs, states = [], []
    for o, row in zip(outs, rows):
        xs.append(x.reshape(shape))
        states.append((P.reshape(shape), H.reshape((3,) + shape)))
        x, P, H = emulate(x, f(o), None, P, H, torch.tensor(row, dtype=torch.float32), 1.0, 0.0)
    E = PB.accumulated(xs, states, outs, rows, 1.0, 0.0, cfg=False)
    y, Q, ets = x0.double(), None, []
    for i, (o, row) in enumerate(zip(outs, rows)):
        a, b, p, q, w0, w1, w2, w3 = row[:8]
        e = o.double()
        if i != 1:
            ets.append(e)
        hist = ([e] + ets[::-1])[:4] if i == 1 else ets[::-1][:4]
        m = sum(w * h for w, h in zip((w0, w1, w2, w3), hist))
        S = Q if i == 1 else y
        if i == 0:
            Q = y
        y = a * S + b * (p * S + q * m)
        got = (x if i == 4 else xs[i + 1]).reshape(shape).double()
        ratio = ((got - y).abs() / E[i]).max().item()
        print(f"by hand: after launch {i} {ratio:.3f} of the accumulated bound")
        assert ratio < 1.0 and (E[i] > 0).all()
