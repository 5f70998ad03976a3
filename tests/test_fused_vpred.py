"""The fused device step for v-prediction and guidance rescale, host side (no GPU).

step_coefficients of DDIM (eta = 0) and Euler (no churn) for prediction_type "v_prediction" against the schedulers' own step() in
float64, and the denoising loop of StableDiffusionDenoiser with CFG and guidance_rescale on the emulated device
(tests/abi_emulator_guidance.py): it takes the fused path -- one mi355x_sd_cfg_rescale_axpby per step -- and ends where the generic
loop (fused_update=False) ends, to the bound of tests/guidance_bounds.py accumulated over the steps."""
import numpy as np
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import guidance_bounds as GB
from tests.abi_emulator import Emulator, on_emulator
from tests.abi_emulator_guidance import GuidanceEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
U64 = 2.0 ** -53
# a x + b v against step(v, t, x), both in float64 on the same double coefficients: step() takes at most 17 roundings (its
# coefficient expressions, two products and a sum or difference for each of x0, the derivative / eps and prev), the linear form at
# most 15 (the expressions of a and b, two products, one sum). No coefficient of either form exceeds 1 in magnitude (|dt| <= sigma,
# sqrt(alpha) <= 1), so every intermediate is at most 2 (|x| + |v|) -- 3 (|x| + |v|) for Euler's x + derivative * dt -- and
# |difference| <= 32 * 3 u64 (|x| + |v|) < K_COEF u64 (|x| + |v|).
K_COEF = 100


def _schedulers(prediction_type):
    return ((DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, prediction_type=prediction_type, **SCHED), 20),
            (EulerDiscreteScheduler(prediction_type=prediction_type, **SCHED), 30))


def test_v_prediction_coefficients_equal_step_in_float64():
    g = torch.Generator().manual_seed(0)
    for sch, steps in _schedulers("v_prediction"):
        lin = type(sch)(**vars(sch.config))
        sch.set_timesteps(steps)
        lin.set_timesteps(steps)
        worst = 0.0
        for t in sch.timesteps:
            x = 3.0 * torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
            v = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
            a, b = lin.step_coefficients(t)
            want = sch.step(v, t, x, return_dict=False)[0]
            assert want.dtype == torch.float64
            ratio = ((a * x + b * v - want).abs() / (K_COEF * U64 * (x.abs() + v.abs()))).max().item()
            worst = max(worst, ratio)
            assert ratio < 1.0, (type(sch).__name__, float(t), ratio)
        print(f"{type(sch).__name__} v_prediction: worst |a x + b v - step| / bound {worst:.3f} over {steps} steps")


def test_epsilon_coefficients_and_refusals_are_unchanged():
    for sch, steps in _schedulers("epsilon"):
        sch.set_timesteps(steps)
        for i, t in enumerate(sch.timesteps):
            a, b = sch.step_coefficients(t)
            if isinstance(sch, EulerDiscreteScheduler):
                assert (a, b) == (1.0, float(sch.sigmas[i + 1]) - float(sch.sigmas[i]))
            else:
                a_t, a_prev = (float(v) for v in sch._alphas(int(t)))
                assert (a, b) == ((a_prev / a_t) ** 0.5, (1 - a_prev) ** 0.5 - (a_prev * (1 - a_t) / a_t) ** 0.5)
    for sch in (DDIMScheduler(clip_sample=False, prediction_type="sample"), EulerDiscreteScheduler(prediction_type="sample"),
                DDIMScheduler(clip_sample=True, prediction_type="v_prediction"), DDIMScheduler(clip_sample=True)):
        sch.set_timesteps(10)
        with pytest.raises(NotImplementedError):
            sch.step_coefficients(sch.timesteps[0])


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


@pytest.mark.parametrize("which", ["euler", "ddim"])
def test_fused_rescale_loop_on_the_emulated_device(which):
    """v-prediction, CFG, guidance_rescale = 0.7: the loop calls cfg_rescale_axpby once per step and nothing of the generic path; the
    generic loop, run in float64 on the model outputs the fused loop saw, ends within the accumulated bound -- every element."""
    steps, gs, gr = 4, 7.5, 0.7
    pe, ne, lat0 = _loop_inputs()
    sch = _schedulers("v_prediction")[which == "euler"][0]
    emu = GuidanceEmulator()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    fused = pipe(pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr, latents=lat0.clone(),
                 callback_on_step_end=lambda p, i, t, kw: (xs.append(kw["latents"].clone()), kw)[1])
    assert emu.calls.count("cfg_rescale_axpby") == steps and len(unet.outs) == steps
    if which == "euler":
        assert sch.step_index is None   # (the fused loop never called scheduler.step)
    sigma0 = float(sch.init_noise_sigma)
    xs = [lat0 * sigma0] + xs
    assert torch.equal(xs[-1], fused)
    coef64 = []
    for t in sch.timesteps:
        coef64.append(sch.step_coefficients(t))
    if which == "euler":
        sch._step_index = None
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
        pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr, latents=lat0.double(), fused_update=False)
    assert generic.dtype == torch.float64
    E = GB.accumulated(xs[:-1], unet.outs, coef64, gs, gr, sigma0)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    print(f"{which}: {steps} steps, |fused - generic| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_rescale():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    sch = _schedulers("v_prediction")[1][0]
    kw = dict(num_inference_steps=2, guidance_rescale=0.7)
    # fused_update=False still selects the generic path
    emu = GuidanceEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, guidance_scale=7.5, latents=lat0.clone(), fused_update=False, **kw)
    assert "cfg_rescale_axpby" not in emu.calls
    b = pipe(pe, ne, guidance_scale=7.5, latents=lat0.clone(), **kw)
    assert emu.calls.count("cfg_rescale_axpby") == 2
    assert torch.allclose(a, b, rtol=2e-5, atol=2e-5)   # (the tolerance of test_pipeline's fused-vs-generic test, same loops)
    # without CFG the reference applies no rescale: plain axpby, v-prediction coefficients
    emu.calls.clear()
    c = pipe(pe, guidance_scale=1.0, latents=lat0.clone(), **kw)
    assert "cfg_rescale_axpby" not in emu.calls and emu.calls.count("axpby") == 2
    d = pipe(pe, guidance_scale=1.0, latents=lat0.clone(), fused_update=False, **kw)
    assert torch.allclose(c, d, rtol=2e-5, atol=2e-5)
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=Emulator()), sch)
    e = old(pe, ne, guidance_scale=7.5, latents=lat0.clone(), **kw)
    assert torch.allclose(e, a, rtol=0, atol=0)
    assert np.isfinite(e.numpy()).all()
