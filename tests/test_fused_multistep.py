"""The fused device step for DPM-Solver multistep sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser with
DPMSolverMultistepScheduler on the emulated device (tests/abi_emulator_multistep.py). It takes the fused path -- one
mi355x_sd_multistep_update per step, scheduler.step never called -- and ends where the generic loop ends when that is run in float64 on
the model outputs the fused loop saw, to the bound of tests/multistep_bounds.py accumulated over the steps."""
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import DPMSolverMultistepScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import multistep_bounds as MB
from tests.abi_emulator import Emulator, _flat, on_emulator
from tests.abi_emulator_multistep import MultistepEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay

STEPS = 6


class _History(MultistepEmulator):
    """keeps what the history buffer held before every call (the second error the accumulated bound carries)"""

    def __init__(self):
        super().__init__()
        self.hs = []

    def mi355x_sd_multistep_update(self, x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream):
        self.hs.append(_flat(m_prev, batch * per_sample, torch.float32).clone())
        return super().mi355x_sd_multistep_update(x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _scheduler():
    sch = DPMSolverMultistepScheduler(**MB.SCHED)
    sch.step_calls = 0
    step = sch.step

    def counted(*a, **kw):
        sch.step_calls += 1
        return step(*a, **kw)
    sch.step = counted
    return sch


@pytest.mark.parametrize("which", ["cfg", "cfg_rescale", "no_cfg", "img2img"])
def test_fused_multistep_loop_on_the_emulated_device(which):
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which == "cfg_rescale" else 0.0)
    cfg = gs > 1.0
    pe, ne, lat0 = _loop_inputs()
    sch = _scheduler()
    emu = _History()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=STEPS, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    if which == "img2img":
        run = STEPS // 2
        fused = pipe(pe, ne, image=lat0.clone(), strength=0.5, generator=torch.Generator().manual_seed(7), callback_on_step_end=cb, **kw)
        timesteps = sch.timesteps[STEPS - run:]
        start = pipe.prepare_image_latents(lat0.clone(), timesteps[:1], 2, torch.Generator().manual_seed(7))
    else:
        run, timesteps, start = STEPS, None, lat0
        fused = pipe(pe, ne if cfg else None, latents=lat0.clone(), callback_on_step_end=cb, **kw)
    assert sch.step_calls == 0 and sch.step_index is None            # scheduler.step was never called
    assert emu.calls.count("multistep_update") == run and len(unet.outs) == run
    assert not {"axpby", "cfg_rescale_axpby"} & set(emu.calls)
    xs = [start] + xs
    assert torch.equal(xs[-1], fused) and torch.isfinite(fused).all()
    assert (sch._step_index, sch.lower_order_nums, sch.model_outputs) == (None, 0, [None, None])
    ts = sch.timesteps if timesteps is None else timesteps
    coef64 = [sch.multistep_coefficients(t) for t in ts]
    sch.set_timesteps(STEPS)
    assert coef64[0][4] == 0.0 and coef64[-1][4] == 0.0 and all(c[4] != 0.0 for c in coef64[1:-1])
    if which == "img2img":   # (the pipeline's own img2img start is cast to fp32: its lines, driven here in float64)
        generic = MB.generic_loop(sch, ts, start, unet.outs, gs, gr, cfg)
    else:
        generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
            pe, ne if cfg else None, latents=lat0.double(), fused_update=False, **kw)
    assert generic.dtype == torch.float64 and sch.step_calls == run
    hs = [h.reshape(lat0.shape) for h in emu.hs]
    E = MB.accumulated(xs[:-1], hs, unet.outs, coef64, gs, gr, cfg)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    print(f"{which}: {run} steps, |fused - generic| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_multistep_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=3, guidance_scale=7.5)
    # fused_update=False and eta select the generic path
    sch, emu = _scheduler(), MultistepEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), fused_update=False, **kw)
    assert "multistep_update" not in emu.calls and sch.step_calls == 3
    pipe(pe, ne, latents=lat0.clone(), eta=0.5, **kw)
    assert "multistep_update" not in emu.calls and sch.step_calls == 6
    b = pipe(pe, ne, latents=lat0.clone(), **kw)
    assert emu.calls.count("multistep_update") == 3 and sch.step_calls == 6
    assert torch.allclose(a, b, rtol=2e-5, atol=2e-5)   # (the tolerance of test_pipeline's fused-vs-generic test, same loops)
    # a callback that replaces the latents leaves the history alone, as the generic loop does
    swap = lambda p, i, t, k: {"latents": k["latents"] * 0.5}  # noqa: E731
    c = pipe(pe, ne, latents=lat0.clone(), callback_on_step_end=swap, **kw)
    d = pipe(pe, ne, latents=lat0.clone(), callback_on_step_end=swap, fused_update=False, **kw)
    assert torch.allclose(c, d, rtol=2e-5, atol=2e-5)
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch2 = _scheduler()
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=Emulator()), sch2)
    e = old(pe, ne, latents=lat0.clone(), **kw)
    assert sch2.step_calls == 3 and torch.equal(e, a)
