"""The bound of tests/multistep_bounds.py and DPMSolverMultistepScheduler.multistep_coefficients, checked on the CPU.

The fp32 restatement of the device kernel in its own order (tests/abi_emulator_multistep.py emulate) stays under the bound on every
case the GPU test runs; three deliberately wrong restatements land above it -- the regrouped (B + D) m0 - D m1 on a row with a large
D, 0 * NaN instead of the skipped history read, a one-pass variance on the offset case. multistep_coefficients reproduces step() in
float64 over full loops of every DPM-Solver configuration of tests/test_reference_modules.py and leaves the scheduler as
set_timesteps left it. Ratios are printed (pytest -s)."""
import numpy as np
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import DPMSolverMultistepScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import multistep_bounds as MB
from tests.abi_emulator import on_emulator
from tests.abi_emulator_multistep import MultistepEmulator, emulate
from tests.configs import TINY
from tests.rowmap_bounds import check

OFFSET = "b2 n4092 offset 64"
U64 = 2.0 ** -53


def _ratios(v, out, m0):
    r = MB.multistep_update(v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"])
    assert torch.isfinite(r["e_out"]).all() and torch.isfinite(r["e_m0"]).all()
    return check(out, r["out"], r["e_out"]), check(m0, r["m0"], r["e_m0"])


@pytest.mark.parametrize("name", list(MB.CASES))
def test_emulation_inside_the_bound(name):
    v = MB.inputs(name)
    ro, rm = _ratios(v, *emulate(v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"]))
    print(f"{name:<36} out err/bound {ro:.3f}  m_out err/bound {rm:.3f}")
    assert ro < 1.0 and rm < 1.0


def test_the_real_rows_are_a_second_order_and_a_first_order_step():
    assert len(MB.ROWS) == 20 and MB.MID[4] != 0.0 and MB.FIRST[4] == 0.0
    assert all(np.isfinite(r).all() for r in MB.ROWS)
    shapes = {(s["batch"], s["n"]) for s in MB.CASES.values()}
    assert {(1, 1), (1, 2), (1, 252), (3, 4092), (3, 4093), (2, 4096), (2, MB.RESIDENT + 4), (8, 65536)} <= shapes


def test_regrouped_difference_is_outside_the_bound():
    """D carries 1 / r: on a row with D = 400 B and a history close to m0, (B + D) m0 - D m1 rounds at |D| |m0| where the reference
    form rounds at |D| |m0 - m1|. The reference form on the same row stays inside. (The regrouped form cannot land far outside:
    the bound already holds |D| e_m0 >= 2 u |D| |m0| for the computed m0 entering the difference.)"""
    v = MB.inputs("b2 n4096 gr0")
    p, q, A, B, D = MB.MID
    v["coef"] = torch.tensor([p, q, A, B, 400.0 * B], dtype=torch.float32)
    m0 = MB.multistep_update(v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"])["m0"]
    v["m1"] = (m0 * (1 + 1e-4 * torch.randn(m0.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64))).float()
    args = (v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"])
    good, _ = _ratios(v, *emulate(*args))
    bad, _ = _ratios(v, *emulate(*args, fault="regroup"))
    print(f"D = 400 B, m1 = m0 (1 + 1e-4 N): reference form {good:.3f}, regrouped form {bad:.3g}")
    assert good < 1.0 < bad


def test_zero_times_nan_is_outside_the_bound():
    v = MB.inputs("b2 n4096 gr0 D0 NaN history")
    args = (v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"])
    good, _ = _ratios(v, *emulate(*args))
    bad, _ = _ratios(v, *emulate(*args, fault="mul_nan"))
    print(f"D = 0, NaN history: skipped read {good:.3f}, 0 * NaN {bad}")
    assert good < 1.0 and bad == float("inf")


def test_one_pass_variance_is_outside_the_bound():
    v = MB.inputs(OFFSET)
    args = (v["x"], v["eu"], v["et"], v["m1"], v["coef"], v["gs"], v["gr"])
    good, gm = _ratios(v, *emulate(*args))
    bad, bm = _ratios(v, *emulate(*args, fault="one_pass"))
    print(f"offset case: two-pass {good:.3f} / {gm:.3f}, one-pass fp32 variance {bad:.3g} / {bm:.3g}")
    assert good < 1.0 and gm < 1.0 and bad > 1.0 and bm > 1.0


# every DPM-Solver configuration of tests/test_reference_modules.py _PRODUCT_SCHEDULERS, and lower_order_final below 15 steps
CONFIGS = {
    "dpmpp_2m": (dict(), 20),
    "dpmpp_2m_karras_heun": (dict(use_karras_sigmas=True, solver_type="heun"), 12),
    "dpm_order1_leading": (dict(algorithm_type="dpmsolver", solver_order=1, timestep_spacing="leading", steps_offset=1), 10),
    "dpmpp_v_prediction": (dict(prediction_type="v_prediction"), 12),
    "dpmpp_sample_prediction_euler_final": (dict(prediction_type="sample", euler_at_final=True, timestep_spacing="trailing"), 16),
    "dpmpp_2m_lower_order_final": (dict(), 10),
    "dpm_2m_heun_sample": (dict(algorithm_type="dpmsolver", solver_type="heun", prediction_type="sample"), 14),
    "dpm_2m_midpoint_v": (dict(algorithm_type="dpmsolver", prediction_type="v_prediction"), 20),
    "dpmpp_2m_karras_midpoint_20": (dict(use_karras_sigmas=True), 20),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_multistep_coefficients_equal_step_in_float64(name):
    """a full loop on float64 tensors through step(); at every step the five-number form on the same sample, model output and
    history: both sides do at most about ten float64 roundings on the terms of the bound"""
    kw, steps = CONFIGS[name]
    sch, lin = DPMSolverMultistepScheduler(**kw), DPMSolverMultistepScheduler(**kw)
    sch.set_timesteps(steps)
    lin.set_timesteps(steps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    worst, orders = 0.0, []
    for t in sch.timesteps:
        e = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        p, q, A, B, D = lin.multistep_coefficients(t)
        m1 = sch.model_outputs[-1]
        want = sch.step(e, t, x, return_dict=False)[0]
        assert want.dtype == torch.float64
        m0 = p * x + q * e
        got = A * x + B * m0
        bound = (A * x).abs() + (B * m0).abs()
        if D != 0.0:
            got = got + D * (m0 - m1)
            bound = bound + abs(D) * (m0.abs() + m1.abs())
        ratio = ((got - want).abs() / (32 * U64 * bound)).max().item()
        worst = max(worst, ratio)
        orders.append(1 if D == 0.0 else 2)
        assert ratio < 1.0, (name, int(t), ratio)
        assert (lin.step_index, lin.lower_order_nums) == (sch.step_index, sch.lower_order_nums)
        x = want
    print(f"{name:<40} worst |five-number form - step| / bound {worst:.3f} over {steps} steps, orders {orders}")
    assert orders[0] == 1
    if kw.get("solver_order", 2) == 1:
        assert set(orders) == {1}
    else:
        assert 2 in orders
    if steps < 15 or kw.get("euler_at_final"):
        assert orders[-1] == 1   # lower_order_final / euler_at_final


def _pipe(sch, backend):
    return StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=backend), sch)


def _state(sch):
    return sch._step_index, sch.lower_order_nums, list(sch.model_outputs), sch.timesteps.tolist(), sch.sigmas.tolist()


def test_fused_plan_leaves_the_scheduler_as_set_timesteps_left_it():
    sch, fresh = DPMSolverMultistepScheduler(**MB.SCHED), DPMSolverMultistepScheduler(**MB.SCHED)
    sch.set_timesteps(8)
    fresh.set_timesteps(8)
    plan = _pipe(sch, MultistepEmulator())._fused_plan(False, "cpu", sch.timesteps[3:])
    assert plan is not None and plan.scales is None and tuple(plan.coef.shape) == (5, 5) and plan.coef.dtype == torch.float32
    assert _state(sch) == _state(fresh)
    # the history starts empty at the first step RUN; 8 < 15 steps: lower_order_final
    assert plan.coef[0, 4] == 0.0 and (plan.coef[1:-1, 4] != 0.0).all() and plan.coef[-1, 4] == 0.0


def test_heun_on_a_long_karras_schedule_keeps_the_generic_path():
    """>= 15 steps: no lower_order_final, the last step is second order on the repeated last sigma: h = 0, heun's 0 / 0"""
    sch = DPMSolverMultistepScheduler(use_karras_sigmas=True, solver_type="heun", **MB.SCHED)
    sch.set_timesteps(16)
    with pytest.raises(NotImplementedError):
        for t in sch.timesteps:
            sch.multistep_coefficients(t)
    sch.set_timesteps(16)
    fresh = DPMSolverMultistepScheduler(use_karras_sigmas=True, solver_type="heun", **MB.SCHED)
    fresh.set_timesteps(16)
    emu = MultistepEmulator()
    pipe = _pipe(sch, emu)
    assert pipe._fused_plan(False, "cpu", sch.timesteps) is None
    assert _state(sch) == _state(fresh)
    g = torch.Generator().manual_seed(0)
    pe, lat0 = torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    with np.errstate(invalid="ignore"):
        pipe(pe, guidance_scale=1.0, num_inference_steps=16, latents=lat0)
    assert "multistep_update" not in emu.calls and sch.step_index == 16   # scheduler.step ran every step
