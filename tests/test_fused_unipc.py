"""The fused device step for UniPC sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser with
UniPCMultistepScheduler on the emulated device (tests/abi_emulator_unipc.py). It takes the fused path -- one mi355x_sd_unipc_update
per step, scheduler.step never called -- and ends where the generic loop ends when that is run in float64 on the model outputs the
fused loop saw, to the bound of tests/unipc_bounds.py accumulated over the steps."""
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import UniPCMultistepScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import unipc_bounds as UB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_multistep import MultistepEmulator
from tests.abi_emulator_unipc import UniPCEmulator
from tests.configs import TINY
from tests.multistep_bounds import generic_loop
from tests.step_pieces import Recording, Replay

STEPS = 8


class _State(UniPCEmulator):
    """keeps what last and the history planes held before every call (the errors the accumulated bound carries) and the pointers"""

    def __init__(self):
        super().__init__()
        self.lasts, self.hists, self.ptrs = [], [], set()

    def mi355x_sd_unipc_update(self, x, eu, et, last, hist, order, out, coef, gs, gr, batch, per_sample, stream):
        n = batch * per_sample
        self.lasts.append(_flat(last, n, torch.float32).clone())
        self.hists.append(_flat(hist, n * order, torch.float32).clone())
        self.ptrs.add((last, hist, order))
        return super().mi355x_sd_unipc_update(x, eu, et, last, hist, order, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _scheduler(**kw):
    sch = UniPCMultistepScheduler(**UB.SCHED, **kw)
    sch.step_calls = 0
    step = sch.step

    def counted(*a, **k):
        sch.step_calls += 1
        return step(*a, **k)
    sch.step = counted
    return sch


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("which", ["cfg", "cfg_rescale", "no_cfg", "img2img"])
def test_fused_unipc_loop_on_the_emulated_device(which, order):
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which == "cfg_rescale" else 0.0)
    cfg = gs > 1.0
    pe, ne, lat0 = _loop_inputs()
    sch = _scheduler(solver_order=order)
    emu = _State()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=STEPS, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    if which == "img2img":
        run = int(STEPS * 0.7)
        fused = pipe(pe, ne, image=lat0.clone(), strength=0.7, generator=torch.Generator().manual_seed(7), callback_on_step_end=cb, **kw)
        timesteps = sch.timesteps[STEPS - run:]
        start = pipe.prepare_image_latents(lat0.clone(), timesteps[:1], 2, torch.Generator().manual_seed(7))
    else:
        run, timesteps, start = STEPS, None, lat0
        fused = pipe(pe, ne if cfg else None, latents=lat0.clone(), callback_on_step_end=cb, **kw)
    assert sch.step_calls == 0 and sch.step_index is None            # scheduler.step was never called
    assert emu.calls.count("unipc_update") == run and len(unet.outs) == run
    assert not {"axpby", "cfg_rescale_axpby", "multistep_update"} & set(emu.calls)
    assert len(emu.ptrs) == 1 and next(iter(emu.ptrs))[2] == order   # one last, one hist for the whole loop
    xs = [start] + xs
    assert torch.equal(xs[-1], fused) and torch.isfinite(fused).all()
    assert (sch._step_index, sch.lower_order_nums, sch.model_outputs, sch.last_sample) == (None, 0, [None] * order, None)
    ts = sch.timesteps if timesteps is None else timesteps
    coef64 = [sch.unipc_coefficients(t) for t in ts]
    sch.set_timesteps(STEPS)
    assert coef64[0][11] == 0.0 and all(c[11] == 1.0 for c in coef64[1:])
    assert coef64[0][9] == 0.0 == coef64[-1][9] and all(c[9] != 0.0 for c in coef64[1:-1])
    if which == "img2img":   # (the pipeline's own img2img start is cast to fp32: its lines, driven here in float64)
        generic = generic_loop(sch, ts, start, unet.outs, gs, gr, cfg)
    else:
        generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
            pe, ne if cfg else None, latents=lat0.double(), fused_update=False, **kw)
    assert generic.dtype == torch.float64 and sch.step_calls == run
    lasts = [v.reshape(lat0.shape) for v in emu.lasts]
    hists = [v.reshape((order,) + tuple(lat0.shape)) for v in emu.hists]
    E = UB.accumulated(xs[:-1], lasts, hists, unet.outs, coef64, gs, gr, order, cfg)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    print(f"{which} order {order}: {run} steps, |fused - generic| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_unipc_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=4, guidance_scale=7.5)
    # fused_update=False selects the generic path
    sch, emu = _scheduler(), UniPCEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), fused_update=False, **kw)
    assert "unipc_update" not in emu.calls and sch.step_calls == 4
    pipe(pe, ne, latents=lat0.clone(), **kw)
    assert emu.calls.count("unipc_update") == 4 and sch.step_calls == 4
    # a callback that replaces the latents leaves last_sample and the history alone, as the generic loop does: the fused loop against
    # the generic one in float64 on the model outputs the fused loop saw, to the accumulated bound (which carries the latents' error
    # through the halving unscaled: an over-estimate)
    sch3, emu3 = _scheduler(), _State()
    unet3 = Recording(on_emulator(UNet2DConditionModel, TINY, P, backend=emu3))
    xs = [lat0]

    def swap(p, i, t, k):
        xs.append(k["latents"] * 0.5)
        return {"latents": xs[-1]}
    c = StableDiffusionDenoiser(unet3, sch3)(pe, ne, latents=lat0.clone(), callback_on_step_end=swap, **kw)
    assert emu3.calls.count("unipc_update") == 4 and sch3.step_calls == 0
    coef64 = [sch3.unipc_coefficients(t) for t in sch3.timesteps]
    sch3.set_timesteps(4)
    d = StableDiffusionDenoiser(Replay(unet3.config, unet3.outs), sch3)(
        pe, ne, latents=lat0.double(), callback_on_step_end=lambda p, i, t, k: {"latents": k["latents"] * 0.5}, fused_update=False, **kw)
    assert d.dtype == torch.float64 and sch3.step_calls == 4
    E = UB.accumulated(xs[:-1], [v.reshape(lat0.shape) for v in emu3.lasts], [v.reshape((2,) + tuple(lat0.shape)) for v in emu3.hists],
                       unet3.outs, coef64, 7.5, 0.0, 2)
    ratio = ((c.double() - d).abs() / E[-1]).max().item()
    print(f"latents halved by the callback after every step: |fused - generic| / accumulated bound {ratio:.3f}")
    assert ratio < 1.0
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch2 = _scheduler()
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=MultistepEmulator()), sch2)
    e = old(pe, ne, latents=lat0.clone(), **kw)
    assert sch2.step_calls == 4 and torch.equal(e, a)
