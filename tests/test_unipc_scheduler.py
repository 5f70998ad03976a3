"""UniPCMultistepScheduler on the CPU: the class reproduces the reference's own sampling loops (tests/golden/unipc, written by
scripts/make_unipc_golden.py), ``unipc_coefficients`` is ``step`` as a linear map (every configuration, with and without the
corrector, in float64), and what is not implemented is refused."""
import numpy as np
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import UniPCMultistepScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import unipc_bounds as UB
from tests import unipc_cases as UC
from tests.abi_emulator import on_emulator
from tests.abi_emulator_unipc import UniPCEmulator
from tests.configs import TINY

U64 = 2.0 ** -53


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("name", list(UC.CONFIGS))
def test_product_class_reproduces_the_reference_sampling_loop(name):
    """the figures of test_product_schedulers_reproduce_the_reference_sampling_loops: timesteps to 1e-6, latents to 2e-5 relative"""
    kw, steps, first = UC.CONFIGS[name]
    gold = np.load(UC.golden_path(name))
    lat, ts = UC.toy_loop(UniPCMultistepScheduler(**UC.SD, **kw), steps, first)
    rt, rl = _rel(torch.tensor(ts), torch.from_numpy(gold["timesteps"])), _rel(lat, torch.from_numpy(gold["latents"]))
    print(f"{name:<30} timesteps {rt:.2g}  latents {rl:.3g}")
    assert rt < 1e-6
    assert rl < 2e-5, rl


# every golden configuration, the corrector switched off at some and at all steps, and the orders on a Karras schedule without
# lower_order_final (the repeated last sigma: h = 0 at the last step)
LINEAR = dict({k: (v[0], v[1], v[2]) for k, v in UC.CONFIGS.items()}, **{
    "corrector_off_everywhere": (dict(solver_order=3, disable_corrector=list(range(12))), 12, 0),
    "corrector_off_some_bh1_v": (dict(solver_order=3, solver_type="bh1", prediction_type="v_prediction", disable_corrector=[1, 2, 5]), 9, 0),
    "eps_prediction_sample_order3": (dict(solver_order=3, predict_x0=False, prediction_type="sample"), 8, 0),
    "eps_prediction_v_karras": (dict(predict_x0=False, prediction_type="v_prediction", use_karras_sigmas=True), 8, 0),
    "karras_order2_no_lower_final": (dict(use_karras_sigmas=True, lower_order_final=False), 8, 0),
    "karras_order3": (dict(use_karras_sigmas=True, solver_order=3), 16, 0),
    "img2img_order3": (dict(solver_order=3), 10, 4),
})


@pytest.mark.parametrize("name", list(LINEAR))
def test_unipc_coefficients_equal_step_in_float64(name):
    """a full loop on float64 tensors through step(); at every step the 12-number form on the same x, e, last_sample and history. Both
    sides round in float64 only, at the magnitudes of the terms: a few dozen roundings on |coefficient| (|a| + |b|) per term."""
    kw, steps, first = LINEAR[name]
    sch, lin = UniPCMultistepScheduler(**UC.SD, **kw), UniPCMultistepScheduler(**UC.SD, **kw)
    sch.set_timesteps(steps)
    lin.set_timesteps(steps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    nan = torch.full_like(x, float("nan"))
    worst, orders, corrs = 0.0, [], []
    for t in sch.timesteps[first:]:
        e = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        k = dict(zip(UB.NAMES, lin.unipc_coefficients(t)))
        L = sch.last_sample if sch.last_sample is not None else nan
        h = [m if m is not None else nan for m in reversed(sch.model_outputs)] + [nan, nan]   # h1, h2, h3: unset ones are NaN
        i, prev_order = (sch.step_index if sch.step_index is not None else first), sch.this_order
        want = sch.step(e, t, x, return_dict=False)[0]
        assert want.dtype == torch.float64
        mt = k["p"] * x + k["q"] * e
        xc, bound = x, torch.zeros_like(x)
        if k["corr"] != 0.0:
            xc = k["Ac"] * L + k["Bc"] * h[0]
            bound = (k["Ac"] * L).abs() + (k["Bc"] * h[0]).abs()
            for n, j in (("C2", 1), ("C3", 2)):
                if k[n] != 0.0:
                    xc = xc + k[n] * (h[j] - h[0])
                    bound = bound + abs(k[n]) * (h[j].abs() + h[0].abs())
            xc = xc + k["Ct"] * (mt - h[0])
            bound = bound + abs(k["Ct"]) * (mt.abs() + h[0].abs())
        got = k["Ap"] * xc + k["Bp"] * mt
        bound = abs(k["Ap"]) * (bound + xc.abs()) + (k["Bp"] * mt).abs()
        for n, j in (("D1", 0), ("D2", 1)):
            if k[n] != 0.0:
                got = got + k[n] * (h[j] - mt)
                bound = bound + abs(k[n]) * (h[j].abs() + mt.abs())
        ratio = ((got - want).abs() / (64 * U64 * bound)).max().item()
        worst = max(worst, ratio)
        assert ratio < 1.0, (name, int(t), ratio)
        assert torch.equal(sch.last_sample, xc) or ((sch.last_sample - xc).abs() <= 64 * U64 * bound).all()
        # the state the walk keeps is the state step() keeps, and the row's zeros are the terms the reference does not form
        assert (lin.step_index, lin.lower_order_nums, lin.this_order) == (sch.step_index, sch.lower_order_nums, sch.this_order)
        corr = i > 0 and i - 1 not in kw.get("disable_corrector", []) and L is not nan
        assert k["corr"] == (1.0 if corr else 0.0)
        c_order = prev_order if corr else 0
        assert (k["Ac"] != 0.0, k["Bc"] != 0.0, k["Ct"] != 0.0) == (corr, corr, corr)
        assert c_order >= 2 or k["C2"] == 0.0
        assert (k["C3"] != 0.0) == (c_order == 3)
        assert sch.this_order >= 2 or k["D1"] == 0.0
        assert (k["D2"] != 0.0) == (sch.this_order == 3)
        orders.append(sch.this_order)
        corrs.append(int(k["corr"]))
        x = want
    print(f"{name:<32} worst |12-number form - step| / bound {worst:.3f} over {len(orders)} steps, orders {orders}, corrector {corrs}")
    assert orders[0] == 1 and corrs[0] == 0 and max(orders) == min(kw.get("solver_order", 2), len(orders))
    if kw.get("lower_order_final", True):
        assert orders[-1] == 1
    if not kw.get("disable_corrector"):
        assert corrs[1:] == [1] * (len(corrs) - 1)


def _state(sch):
    return (sch._step_index, sch.lower_order_nums, list(sch.model_outputs), list(sch.timestep_list), sch.last_sample, sch.this_order,
            sch.timesteps.tolist(), sch.sigmas.tolist())


def _pipe(sch, backend):
    return StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=backend), sch)


def test_fused_plan_leaves_the_scheduler_as_set_timesteps_left_it():
    sch, fresh = UniPCMultistepScheduler(solver_order=3, **UC.SD), UniPCMultistepScheduler(solver_order=3, **UC.SD)
    sch.set_timesteps(8)
    fresh.set_timesteps(8)
    plan = _pipe(sch, UniPCEmulator())._fused_plan(False, "cpu", sch.timesteps[3:])
    assert plan is not None and plan.scales is None and tuple(plan.coef.shape) == (5, 12) and plan.coef.dtype == torch.float32
    assert plan.order == 3 and _state(sch) == _state(fresh)
    # the state starts empty at the first step RUN: no corrector, first order; then the orders 2, 3, and 2, 1 at the end
    assert (plan.coef[0, 2:7] == 0.0).all() and (plan.coef[0, 9:] == 0.0).all() and (plan.coef[1:, 11] == 1.0).all()
    assert [int((row[9:11] != 0.0).sum()) + 1 for row in plan.coef] == [1, 2, 3, 2, 1]


def test_refusals():
    for kw in (dict(thresholding=True), dict(solver_p=object()), dict(trained_betas=[0.1, 0.2]), dict(solver_order=4),
               dict(solver_type="bh3"), dict(beta_schedule="squaredcos_cap_v2")):
        with pytest.raises(NotImplementedError):
            UniPCMultistepScheduler(**kw)
    assert UniPCMultistepScheduler(solver_type="midpoint").config.solver_type == "bh2"
    sch = UniPCMultistepScheduler()
    with pytest.raises(ValueError):
        sch.step(torch.zeros(1), 0, torch.zeros(1))
    with pytest.raises(ValueError):
        sch.unipc_coefficients(0)


def test_third_order_on_a_karras_schedule_without_lower_order_final_keeps_the_generic_path():
    """The one supported configuration with a non-finite row (every combination of order, solver type, prediction, spacing, Karras
    and lower_order_final was walked at 3, 8 and 20 steps): the Karras schedule repeats its last sigma, so the last step has h = 0;
    without lower_order_final it is a third-order step whose r_k are infinite, and the 2 x 2 solve yields NaN -- in step() too.
    Order 2 survives the same step (rhos_p is the constant 0.5, D1 = 0 / inf = 0), as LINEAR's karras_order2_no_lower_final shows."""
    kw = dict(use_karras_sigmas=True, solver_order=3, lower_order_final=False, **UC.SD)
    sch = UniPCMultistepScheduler(**kw)
    sch.set_timesteps(8)
    for t in sch.timesteps[:-1]:
        assert np.isfinite(sch.unipc_coefficients(t)).all()
    with pytest.raises(NotImplementedError):
        sch.unipc_coefficients(sch.timesteps[-1])
    lat, _ = UC.toy_loop(UniPCMultistepScheduler(**kw), 8)
    assert not torch.isfinite(lat).all()   # the generic step's own answer on this configuration
    sch = UniPCMultistepScheduler(**kw)
    sch.set_timesteps(8)
    fresh = UniPCMultistepScheduler(**kw)
    fresh.set_timesteps(8)
    emu = UniPCEmulator()
    pipe = _pipe(sch, emu)
    assert pipe._fused_plan(False, "cpu", sch.timesteps) is None
    assert _state(sch) == _state(fresh)
    g = torch.Generator().manual_seed(0)
    pe, lat0 = torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    pipe(pe, guidance_scale=1.0, num_inference_steps=8, latents=lat0)
    assert "unipc_update" not in emu.calls and sch.step_index == 8   # scheduler.step ran every step


def test_add_noise_uses_the_sigma_of_the_current_schedule():
    sch = UniPCMultistepScheduler(**UC.SD)
    sch.set_timesteps(10)
    g = torch.Generator().manual_seed(1)
    x, n = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    t = torch.tensor([int(sch.timesteps[3])] * 2)
    a, s = sch._sigma_to_alpha_sigma_t(sch.sigmas[3])
    assert torch.allclose(sch.add_noise(x, n, t), float(a) * x + float(s) * n, rtol=1e-6, atol=1e-6)
    assert len(sch) == 1000 and sch.init_noise_sigma == 1.0 and sch.scale_model_input(x, 5) is x
