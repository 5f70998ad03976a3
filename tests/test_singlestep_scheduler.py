"""DPMSolverSinglestepScheduler on the CPU: the recorded loops of the reference's own class (tests/golden/singlestep, bit for bit),
the configuration surface and its registrations, every refusal, the coefficient walk's state, and ``singlestep_coefficients`` applied
in float64 against ``step`` in float64 on every recorded configuration."""
import math

import numpy as np
import pytest
import torch

from paddlemix_amd.schedulers import _WALKED, DPMSolverSinglestepScheduler
from tests import singlestep_cases as SC

U64 = 2.0 ** -53
S = DPMSolverSinglestepScheduler


@pytest.mark.parametrize("name", list(SC.CONFIGS))
def test_recorded_loop_of_the_reference_bit_for_bit(name):
    kw, steps, first = SC.CONFIGS[name]
    gold = np.load(SC.golden_path(name))
    lat, ts, sigmas, orders = SC.toy_loop(S(**kw), steps, first)
    assert ts == gold["timesteps"].tolist() and orders == gold["order_list"].tolist()
    assert np.array_equal(np.float32(sigmas).view(np.int32), gold["sigmas"].view(np.int32))
    assert lat.dtype == torch.float32 and gold["latents"].dtype == np.float32 and np.isfinite(gold["latents"]).all()
    off = int((lat.numpy().view(np.int32) != gold["latents"].view(np.int32)).sum())
    print(f"{name}: {steps} steps from {first}, orders {orders[first:]}, {off} of {lat.numel()} end latents differ in bits")
    assert off == 0


def test_the_recorded_cases_cover_what_they_must():
    C = SC.CONFIGS
    lists = {n: np.load(SC.golden_path(n))["order_list"].tolist() for n in C}
    assert lists["order2_default"] == [1, 2] * 5 and lists["order2_odd"] == [1, 2, 1, 2, 1, 2, 1]
    assert lists["order3_heun"] == [1, 2, 3] * 3 + [1] and lists["order3_midpoint"] == [1, 2, 3, 1, 2, 3, 1, 2, 1]
    assert lists["order3_no_lower_final"] == [1, 2, 3] * 3 and lists["order3_uneven_no_lower_final"] == [1, 2, 3, 1, 2, 3, 1, 2]
    assert lists["one_step"] == [1] and lists["order1"] == [1] * 6
    assert C["dpmsolver_heun_sample"][0]["prediction_type"] == "sample" and C["karras_v"][0]["use_karras_sigmas"]
    # the img2img starts: an index whose listed order is 2 and one whose listed order is 3 -- both reductions of step
    assert lists["img2img_listed2"][C["img2img_listed2"][2]] == 2 and lists["img2img_listed3"][C["img2img_listed3"][2]] == 3
    assert lists["img2img_order2"][C["img2img_order2"][2]] == 2


@pytest.mark.parametrize("order,lof,steps,want", [
    (1, True, 5, [1] * 5), (1, False, 5, [1] * 5), (2, True, 6, [1, 2] * 3), (2, True, 7, [1, 2] * 3 + [1]), (2, False, 6, [1, 2] * 3),
    (3, True, 9, [1, 2, 3, 1, 2, 3, 1, 2, 1]), (3, True, 10, [1, 2, 3] * 3 + [1]), (3, True, 11, [1, 2, 3] * 3 + [1, 2]),
    (3, False, 9, [1, 2, 3] * 3), (3, True, 3, [1, 2, 1]), (3, True, 1, [1]), (3, True, 2, [1, 2])])
def test_get_order_list(order, lof, steps, want):
    sch = S(solver_order=order, lower_order_final=lof)
    assert sch.get_order_list(steps) == want
    sch.set_timesteps(steps)
    assert sch.order_list == want and len(sch.timesteps) == steps and len(sch.sigmas) == steps + 1


def test_config_surface_and_registrations():
    sch = S()
    c = sch.config
    assert (c.num_train_timesteps, c.beta_start, c.beta_end, c.beta_schedule, c.trained_betas, c.solver_order) == \
        (1000, 0.0001, 0.02, "linear", None, 2)
    assert (c.prediction_type, c.thresholding, c.dynamic_thresholding_ratio, c.sample_max_value) == ("epsilon", False, 0.995, 1.0)
    assert (c.algorithm_type, c.solver_type, c.lower_order_final, c.use_karras_sigmas, c.variance_type) == \
        ("dpmsolver++", "midpoint", True, False, None)
    assert c.lambda_min_clipped == -float("inf") and not hasattr(c, "timestep_spacing") and not hasattr(c, "steps_offset")
    assert sch.order == 1 and sch.init_noise_sigma == 1.0 and len(sch) == 1000 and sch.step_index is None
    assert sch.model_outputs == [None, None] and sch.sample is None and sch.num_inference_steps is None
    assert len(sch.timesteps) == 1000 and sch.timesteps[0] == 999 and len(sch.order_list) == 1000
    x = torch.randn(1, 4, 8, 8)
    assert sch.scale_model_input(x, 3) is x
    assert S(algorithm_type="deis").config.algorithm_type == "dpmsolver++"
    assert S(algorithm_type="dpmsolver").config.algorithm_type == "dpmsolver"
    for st in ("logrho", "bh1", "bh2"):
        assert S(solver_type=st).config.solver_type == "midpoint"
    assert S(solver_type="heun").config.solver_type == "heun"
    # an uneven step count switches lower_order_final on, for good (the reference registers it in the config)
    sch = S(solver_order=3, lower_order_final=False)
    sch.set_timesteps(9)
    assert sch.config.lower_order_final is False
    sch.set_timesteps(8)
    assert sch.config.lower_order_final is True and sch.order_list == [1, 2, 3, 1, 2, 3, 1, 2]
    # set_timesteps puts the step state back
    sch.step(x, sch.timesteps[0], x)
    assert sch.step_index == 1 and sch.sample is x
    sch.set_timesteps(8)
    assert sch.step_index is None and sch.sample is None and sch.model_outputs == [None] * 3


def test_refusals():
    for kw in (dict(thresholding=True), dict(trained_betas=[0.1, 0.2]), dict(lambda_min_clipped=-5.1), dict(variance_type="learned"),
               dict(variance_type="learned_range"), dict(solver_order=4), dict(solver_order=0)):
        with pytest.raises(NotImplementedError, match=r"DPMSolverSinglestepScheduler\(mi355x\)"):
            S(**kw)
    for kw, word in ((dict(algorithm_type="sde-dpmsolver++"), "sde-dpmsolver\\+\\+"), (dict(solver_type="euler"), "euler"),
                     (dict(beta_schedule="squaredcos_cap_v2"), "squaredcos_cap_v2")):
        with pytest.raises(NotImplementedError, match=word):
            S(**kw)
    sch = S()
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.step(x, 999, x)
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.singlestep_coefficients(999)
    sch = S(prediction_type="velocity")
    sch.set_timesteps(4)
    with pytest.raises(ValueError, match="prediction_type given as velocity"):
        sch.step(x, sch.timesteps[0], x)
    with pytest.raises(NotImplementedError):
        sch.singlestep_coefficients(sch.timesteps[0])
    with pytest.raises(ValueError, match="sample"):
        S().convert_model_output(x)


def test_add_noise_uses_the_current_schedule():
    sch = S(**SC.SD)
    sch.set_timesteps(10)
    g = torch.Generator().manual_seed(1)
    x0, n = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    t = sch.timesteps[3]
    got = sch.add_noise(x0, n, torch.tensor([t, t]))
    s = float(sch.sigmas[3])
    a = 1 / math.sqrt(s * s + 1)
    assert torch.allclose(got, a * x0 + s * a * n, rtol=1e-6, atol=1e-6)


def _state(sch):
    return sch._step_index, list(sch.model_outputs), sch.sample, sch._last_order, sch.timesteps.tolist(), sch.sigmas.tolist(), \
        list(sch.order_list), vars(sch.config)


@pytest.mark.parametrize("name", list(SC.CONFIGS))
def test_coefficient_walk_leaves_the_scheduler_as_set_timesteps_left_it(name):
    kw, steps, first = SC.CONFIGS[name]
    sch, fresh = S(**kw), S(**kw)
    sch.set_timesteps(steps)
    fresh.set_timesteps(steps)
    with sch.coefficient_walk():
        rows = [sch.singlestep_coefficients(t) for t in sch.timesteps[first:]]
        assert sch.step_index == steps and sch.sample is _WALKED and all(m is _WALKED for m in sch.model_outputs[-min(2, len(rows)):])
    assert _state(sch) == _state(fresh)
    assert all(len(r) == 8 and all(map(math.isfinite, r)) for r in rows)
    # the effective orders: the list's, lowered at an img2img start; keep exactly where an order-3 row follows an order-2 one
    orders = [int(r[6]) for r in rows]
    listed = sch.order_list[first:]
    assert orders[0] == 1 and all(o == w or (i < 2 and o < w) for i, (o, w) in enumerate(zip(orders, listed)))
    assert all(o == 1 or o == orders[i - 1] + 1 for i, o in enumerate(orders))    # order k > 1 directly follows order k - 1
    assert [r[7] for r in rows] == [float(o == 2 and i + 1 < len(orders) and orders[i + 1] == 3) for i, o in enumerate(orders)]
    assert all((r[5] != 0.0) == (o == 3 and sch.config.solver_type == "heun") for r, o in zip(rows, orders))
    assert all((r[4] != 0.0) == (o > 1) for r, o in zip(rows, orders))


@pytest.mark.parametrize("name", list(SC.CONFIGS))
def test_singlestep_coefficients_equal_step_in_float64(name):
    """the recorded configuration's loop on float64 tensors through step(); at every evaluation the row applied in float64 to the same
    sample, model output, parked sample and group outputs: both sides do a few float64 roundings on the terms of the bound"""
    kw, steps, first = SC.CONFIGS[name]
    sch, lin = S(**kw), S(**kw)
    lin.set_timesteps(steps)
    seen = []
    SC.toy_loop(sch, steps, first, dtype=torch.float64, seen=seen)
    sch.set_timesteps(steps)
    worst, park, base, m1, base_mag, m1_mag = 0.0, None, None, None, None, None
    for t, (x, e) in zip(sch.timesteps[first:], seen):
        p, q, A, B, E1, E2, order, keep = lin.singlestep_coefficients(t)
        want = sch.step(e, t, x, return_dict=False)[0]
        assert want.dtype == torch.float64
        m0, mag = p * x + q * e, (p * x).abs() + (q * e).abs()   # (mag: what m0's own roundings scale with, on both sides)
        if order == 1.0:
            park, base, base_mag = x, m0, mag
            got, bound = A * x + B * m0, (A * x).abs() + abs(B) * mag
        else:
            got = A * park + B * base + E1 * (m0 - base)
            bound = (A * park).abs() + abs(B) * base_mag + abs(E1) * (mag + base_mag)
            if order == 3.0 and E2 != 0.0:
                got = got + E2 * (m1 - base)
                bound = bound + abs(E2) * (m1_mag + base_mag)
            if keep:
                m1, m1_mag = m0, mag
        ratio = ((got - want).abs() / (64 * U64 * bound)).max().item()
        worst = max(worst, ratio)
        assert ratio < 1.0, (name, int(t), order, ratio)
        assert lin.step_index == sch.step_index and lin._last_order == sch._last_order == int(order)
    print(f"{name:<32} worst |row form - step| / bound {worst:.3f} over {len(seen)} evaluations")


def test_a_row_that_is_not_finite_raises_and_leaves_the_state():
    """two sigmas made equal across an order-2 step: h = 0, heun's 0 / 0 (where step itself yields NaN)"""
    sch = S(solver_type="heun", **SC.SD)
    sch.set_timesteps(6)
    sch.sigmas[4] = sch.sigmas[2]   # the order-2 evaluation at index 3 steps from sigma index 2 to 4
    with sch.coefficient_walk():
        for t in sch.timesteps[:3]:
            sch.singlestep_coefficients(t)
        before = _state(sch)
        with pytest.raises(NotImplementedError, match="not finite"):
            sch.singlestep_coefficients(sch.timesteps[3])
        assert _state(sch) == before
    assert sch.step_index is None and sch.model_outputs == [None, None] and sch.sample is None and sch._last_order == 0
    # ... and on the first call of a walk the step index goes back to None
    sch.sigmas[1] = sch.sigmas[0]
    sch.sigmas[2] = sch.sigmas[0]
    sch.order_list = [2] * 6
    sch.model_outputs = [None, _WALKED]
    sch._last_order = 1
    with pytest.raises(NotImplementedError, match="not finite"):
        sch.singlestep_coefficients(sch.timesteps[1])
    assert sch.step_index is None and sch.model_outputs == [None, _WALKED]


def test_the_walk_refuses_what_the_planes_cannot_hold():
    x = torch.randn(1, 4, 8, 8)
    # step has run on this scheduler: its history holds tensors the device planes never saw
    sch = S(**SC.SD)
    sch.set_timesteps(6)
    sch.step(x, sch.timesteps[0], x)
    before = _state(sch)
    with pytest.raises(NotImplementedError, match="coefficient walk"):
        sch.singlestep_coefficients(sch.timesteps[1])
    assert _state(sch) == before
    # an order-2 evaluation that does not follow an order-1 one (a state no order list and no img2img start produces)
    sch = S(**SC.SD)
    sch.set_timesteps(6)
    sch.order_list = [1, 2, 2, 2, 1, 2]
    with sch.coefficient_walk():
        sch.singlestep_coefficients(sch.timesteps[0])
        sch.singlestep_coefficients(sch.timesteps[1])
        with pytest.raises(NotImplementedError, match="order-2 evaluation that does not follow an order-1 one"):
            sch.singlestep_coefficients(sch.timesteps[2])
    # thresholding switched on behind the constructor's back
    sch = S(**SC.SD)
    sch.set_timesteps(6)
    sch.config.thresholding = True
    with pytest.raises(NotImplementedError, match="thresholding"):
        sch.singlestep_coefficients(sch.timesteps[0])
    assert sch.step_index is None
