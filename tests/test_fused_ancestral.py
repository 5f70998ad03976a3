"""The fused device step for ancestral Euler sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser with
EulerAncestralDiscreteScheduler on the emulated device (tests/abi_emulator_ancestral.py). It takes the fused path -- one
mi355x_sd_ancestral_update per step, scheduler.step never called -- and ends where the pipeline's own fused_update=False loop ends
under the same generator seed when that is run in float64 on the model outputs the fused loop saw, to the bound of
tests/ancestral_bounds.py accumulated over the steps. (float64 randn draws other numbers than float32 from one seed: the float64 loop's
step is handed the float32 draw of its generator, widened -- counting of tests/step_pieces.py.) The pipeline's unmodified float32 generic loop under the
same seed is run too: it leaves the generator where the fused loop leaves it."""
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser, _AncestralTail
from paddlemix_amd.schedulers import EulerAncestralDiscreteScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import ancestral_bounds as AB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_ancestral import AncestralEmulator
from tests.abi_emulator_multistep import MultistepEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay, counting

STEPS, SEED = 8, 7


class _State(AncestralEmulator):
    """keeps the noise plane and the coefficient row every call was given"""

    def __init__(self):
        super().__init__()
        self.zs, self.rows = [], []

    def mi355x_sd_ancestral_update(self, x, eu, et, noise, out, coef, gs, gr, batch, per_sample, stream):
        assert noise, "the Python tail always passes a real plane"
        self.zs.append(_flat(noise, batch * per_sample, torch.float32).clone())
        self.rows.append(_flat(coef, 3, torch.float32).clone())
        return super().mi355x_sd_ancestral_update(x, eu, et, noise, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _gen():
    return torch.Generator().manual_seed(SEED)


def _scheduler(widen=False, **kw):
    return counting(EulerAncestralDiscreteScheduler(**AB.SCHED, **kw), widen)


@pytest.mark.parametrize("which", ["no_cfg", "cfg", "cfg_rescale", "v_prediction", "img2img", "inpaint"])
def test_fused_ancestral_loop_on_the_emulated_device(which):
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which in ("cfg_rescale", "v_prediction") else 0.0)
    cfg = gs > 1.0
    skw = dict(prediction_type="v_prediction", timestep_spacing="trailing") if which == "v_prediction" else {}
    pe, ne, lat0 = _loop_inputs()
    sch = _scheduler(**skw)
    emu = _State()
    P = synth_unet_params(TINY, seed=1234)
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, P, backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=STEPS, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    mask = (torch.arange(64).reshape(1, 1, 8, 8) % 3 == 0).float().repeat(2, 1, 1, 1)
    if which == "img2img":
        call, run = dict(image=lat0.clone(), strength=0.7), int(STEPS * 0.7)
    elif which == "inpaint":   # a 4-channel UNet: the kept region is re-imposed after every step (add_noise)
        call, run = dict(image=lat0.clone(), mask_image=mask, masked_image_latents=lat0 * (1 - mask)), STEPS
    else:
        call, run = dict(latents=lat0.clone()), STEPS
    g_fused = _gen()
    fused = pipe(pe, ne if cfg else None, generator=g_fused, callback_on_step_end=cb, **call, **kw)
    first = STEPS - run
    assert sch.step_calls == 0 and sch.step_index is None            # scheduler.step was never called, the walk left no state
    assert emu.calls.count("ancestral_update") == run == len(unet.outs)   # once per step
    assert not {"axpby", "cfg_axpby", "cfg_rescale_axpby", "multistep_update", "unipc_update"} & set(emu.calls)
    assert torch.isfinite(fused).all() and torch.equal(xs[-1], fused)
    # the rows the launches read: row i of the table over the WHOLE schedule, the last one without noise
    coef64 = [sch.ancestral_coefficients(t) for t in sch.timesteps]
    sch.set_timesteps(STEPS)
    assert len(coef64) == STEPS and coef64[-1][2] == 0.0 and all(c[2] > 0.0 for c in coef64[:-1])
    coef64 = coef64[first:]
    assert all(torch.equal(r, torch.tensor(c, dtype=torch.float32)) for r, c in zip(emu.rows, coef64))
    # the planes: the generator's draws after whatever the start took, in order, the last step's included
    g = _gen()
    sigma0 = sch.init_noise_sigma
    if which == "img2img":
        start = pipe.prepare_image_latents(lat0.clone(), sch.timesteps[first:][:1], 2, g)
    elif which == "inpaint":
        start = torch.randn(lat0.shape, generator=g) * sigma0
    else:
        start = lat0 * sigma0
    zs = [torch.randn(lat0.shape, generator=g) for _ in range(run)]
    assert all(torch.equal(a.reshape(lat0.shape), b) for a, b in zip(emu.zs, zs))
    assert torch.equal(torch.randn(5, generator=g), torch.randn(5, generator=g_fused))
    # the pipeline's fused_update=False loop, float64 on the recorded model outputs, the same seed
    sch64 = _scheduler(widen=True, **skw)
    if "latents" in call:
        call = dict(latents=lat0.double())
    g64 = _gen()
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(
        pe, ne if cfg else None, generator=g64, fused_update=False, **call, **kw)
    assert generic.dtype == torch.float64 and sch64.step_calls == run
    assert torch.equal(torch.randn(5, generator=g64), torch.randn(5, generator=_after(run, which, pipe, sch, lat0, first)))
    xs = [start] + xs
    E = AB.accumulated(xs[:-1], zs, unet.outs, coef64, gs, gr, cfg, sigma0=sigma0 if "latents" in call else 1.0)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    # and the unmodified float32 generic loop: reported, and it leaves the generator where the fused loop left it
    sch32, g32 = _scheduler(**skw), _gen()
    if "latents" in call:
        call = dict(latents=lat0.clone())
    plain = StableDiffusionDenoiser(Replay(unet.config, unet.outs, dtype=torch.float32), sch32)(
        pe, ne if cfg else None, generator=g32, fused_update=False, **call, **kw)
    assert sch32.step_calls == run and torch.equal(torch.randn(5, generator=g32), torch.randn(5, generator=_after(run, which, pipe, sch, lat0, first)))
    print(f"{which}: {run} steps, |fused - generic float64| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}; |fused - generic float32| / |latent| at most "
          f"{float(((fused - plain).abs() / generic.abs().max()).max()):.2e}")
    assert ratio < 1.0


def _after(run, which, pipe, sch, lat0, first):
    """a generator of the seed, advanced by what one call draws: the start's noise (img2img, inpaint) and one plane per step"""
    g = _gen()
    if which in ("img2img", "inpaint"):
        torch.randn(lat0.shape, generator=g)
    for _ in range(run):
        torch.randn(lat0.shape, generator=g)
    return g


def test_routing_around_the_ancestral_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=4, guidance_scale=7.5)
    # fused_update=False selects the generic path; so does eta != 0
    sch, emu = _scheduler(), AncestralEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), generator=_gen(), fused_update=False, **kw)
    assert "ancestral_update" not in emu.calls and sch.step_calls == 4
    pipe(pe, ne, latents=lat0.clone(), generator=_gen(), eta=0.5, **kw)
    assert "ancestral_update" not in emu.calls and sch.step_calls == 8
    b = pipe(pe, ne, latents=lat0.clone(), generator=_gen(), **kw)
    assert emu.calls.count("ancestral_update") == 4 and sch.step_calls == 8
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4) and not torch.equal(b, pipe(pe, ne, latents=lat0.clone(), generator=torch.Generator().manual_seed(8), **kw))
    # the plan: a table over the whole schedule with the model-input scales, the call's generator, the scheduler left as it was
    sch.set_timesteps(4)
    g = _gen()
    plan = pipe._fused_plan(False, "cpu", sch.timesteps[1:], g)
    assert isinstance(plan, _AncestralTail) and tuple(plan.coef.shape) == (4, 3) and plan.coef.dtype == torch.float32
    assert plan.generator is g and len(plan.scales) == 4 and sch.step_index is None
    assert plan.scales == [1.0 / (float(s) ** 2 + 1) ** 0.5 for s in sch.sigmas[:-1]]
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch2 = _scheduler()
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=MultistepEmulator()), sch2)
    e = old(pe, ne, latents=lat0.clone(), generator=_gen(), **kw)
    assert sch2.step_calls == 4 and torch.equal(e, a)
    # sample prediction has no linear form here: the plan is None and the generic step refuses as the reference does
    sch3 = _scheduler(prediction_type="sample")
    pipe3 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=AncestralEmulator()), sch3)
    with pytest.raises(NotImplementedError, match="sample"):
        pipe3(pe, ne, latents=lat0.clone(), generator=_gen(), **kw)
