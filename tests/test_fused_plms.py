"""The fused device step for PLMS sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser with a stock SD-1.x
PNDMScheduler (skip_prk_steps) on the emulated device (tests/abi_emulator_plms.py). It takes the fused path -- one
mi355x_sd_plms_update per model evaluation, n + 1 of them, scheduler.step never called, the coefficient row advancing by 48 bytes and
the parked sample and the ring at fixed addresses -- and ends where the pipeline's own fused_update=False loop ends when that is run in
float64 on the model outputs the fused loop saw, to the bound of tests/plms_bounds.py accumulated over the launches. Before the entry
existed (ABI 19) the same loop took _GenericTail: the loop test and the ABI-surface test fail there."""
import os
import re

import pytest
import torch

from paddlemix_amd import _lib, ops
from paddlemix_amd import pipeline as PL
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import PNDMScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import plms_bounds as PB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_dpm2 import Dpm2Emulator
from tests.abi_emulator_plms import PlmsEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay, counting

STEPS = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _State(PlmsEmulator):
    """keeps the pointers, the coefficient row, the parked sample and the ring every call was given"""

    def __init__(self):
        super().__init__()
        self.rows, self.ptrs, self.states = [], [], []

    def mi355x_sd_plms_update(self, x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream):
        n = batch * per_sample
        self.rows.append(_flat(coef, 12, torch.float32).clone())
        self.ptrs.append((coef, park, hist))
        self.states.append((_flat(park, n, torch.float32).clone(), _flat(hist, 3 * n, torch.float32).clone()))
        return super().mi355x_sd_plms_update(x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _scheduler(**kw):
    return counting(PNDMScheduler(**dict(PB.SCHED, **kw)))


def _gen():
    return torch.Generator().manual_seed(7)


def test_the_abi_surface_has_the_entry():
    header = open(os.path.join(ROOT, "include", "mi355x_sd.h")).read()
    assert re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", header).group(1) == str(_lib.ABI_VERSION) and _lib.ABI_VERSION >= 20
    decl = re.search(r"int mi355x_sd_plms_update\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["x", "eps_uncond", "eps_text", "park", "hist", "out", "coef", "guidance_scale", "guidance_rescale", "batch",
                     "per_sample", "stream"]
    res, args = _lib.SIGNATURES["mi355x_sd_plms_update"]
    assert len(args) == len(names) and callable(ops.plms_update)
    tail = PL._PlmsTail
    assert tail in PL._TAILS and (tail.walk, tail.entry, tail.whole_schedule) == ("plms_coefficients", "mi355x_sd_plms_update", False)
    assert PL._TAILS.index(tail) < PL._TAILS.index(PL._LinearTail) and hasattr(PNDMScheduler, "plms_coefficients")


@pytest.mark.parametrize("which", ["cfg", "cfg_rescale", "img2img", "no_cfg", "v_prediction"])
def test_fused_plms_loop_on_the_emulated_device(which):
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which in ("cfg_rescale", "v_prediction") else 0.0)
    cfg = gs > 1.0
    skw = dict(prediction_type="v_prediction", timestep_spacing="trailing") if which == "v_prediction" else {}
    pe, ne, lat0 = _loop_inputs()
    sch = _scheduler(**skw)
    emu = _State()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=STEPS, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    if which == "img2img":   # strength 0.7: int(8 * 0.7) = 5 steps kept, the loop starts at index 3 of the 9 timesteps
        call, first = dict(image=lat0.clone(), strength=0.7), 3
    else:
        call, first = dict(latents=lat0.clone()), 0
    run = STEPS + 1 - first
    fused = pipe(pe, ne if cfg else None, generator=_gen(), callback_on_step_end=cb, **call, **kw)
    assert sch.step_calls == 0 and (sch.counter, sch.ets, sch.cur_sample) == (0, [], None)   # step never called, the walk left no state
    assert emu.calls.count("plms_update") == run == len(unet.outs)                            # one launch per model evaluation
    assert not {"axpby", "cfg_axpby", "cfg_rescale_axpby", "multistep_update", "unipc_update", "ancestral_update", "heun_update",
                "dpm2_update"} & set(emu.calls)
    assert torch.isfinite(fused).all() and torch.equal(xs[-1], fused)
    # the rows the launches read: row i - first of a table over the timesteps the loop RUNS, 48 bytes apart; the state never moves
    with sch.coefficient_walk():
        coef64 = [sch.plms_coefficients(t) for t in sch.timesteps[first:]]
    assert len(coef64) == run and [c[10] for c in coef64] == [0.0, 1.0] + [0.0] * (run - 2) and coef64[0][9] == 1.0
    assert all(torch.equal(r, torch.tensor(c, dtype=torch.float32)) for r, c in zip(emu.rows, coef64))
    assert [p[0] - emu.ptrs[0][0] for p in emu.ptrs] == [48 * k for k in range(run)]
    assert len({p[1:] for p in emu.ptrs}) == 1 and emu.ptrs[0][1] != emu.ptrs[0][2]
    # the pipeline's fused_update=False loop, float64 on the recorded model outputs
    if which == "img2img":
        start = pipe.prepare_image_latents(lat0.clone(), sch.timesteps[first:][:1], 2, _gen())
    else:
        start, call = lat0 * sch.init_noise_sigma, dict(latents=lat0.double())
    sch64 = _scheduler(**skw)
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    assert generic.dtype == torch.float64 and sch64.step_calls == run and sch64.counter == run
    xs = [start] + xs
    states = [(P.reshape(lat0.shape), H.reshape((3,) + tuple(lat0.shape))) for P, H in emu.states]
    E = PB.accumulated(xs[:-1], states, unet.outs, coef64, gs, gr, cfg)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    assert sch.timesteps.tolist() == sch64.timesteps.tolist() and sch.num_inference_steps == sch64.num_inference_steps
    # and the unmodified float32 generic loop: reported
    if "latents" in call:
        call = dict(latents=lat0.clone())
    plain = StableDiffusionDenoiser(Replay(unet.config, unet.outs, dtype=torch.float32), _scheduler(**skw))(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    print(f"{which}: {run} launches, |fused - generic float64| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}; |fused - generic float32| / |latent| at most "
          f"{float(((fused - plain).abs() / generic.abs().max()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_plms_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=4, guidance_scale=7.5)
    # fused_update=False selects the generic path
    sch, emu = _scheduler(), PlmsEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), fused_update=False, **kw)
    assert "plms_update" not in emu.calls and sch.step_calls == 5
    b = pipe(pe, ne, latents=lat0.clone(), **kw)
    assert emu.calls.count("plms_update") == 5 and sch.step_calls == 5
    # (a sanity check only: here each loop feeds its own latents to the bf16 UNet, whose operands round at 2^-9; the test above
    # replays the model outputs and holds the fused loop to the float64 bound)
    assert float((a - b).abs().max()) <= 2.0 ** -9 * float(a.abs().max())
    # the plan: a table over the timesteps handed in, no model-input scales, the scheduler left as it was
    sch.set_timesteps(4)
    plan = pipe._fused_plan(False, "cpu", sch.timesteps[2:], None)
    assert isinstance(plan, PL._PlmsTail) and tuple(plan.coef.shape) == (3, 12) and plan.coef.dtype == torch.float32
    assert plan.scales is None and (sch.counter, sch.ets, sch.cur_sample) == (0, [], None)
    assert plan.coef[:, 8:].tolist() == [[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]]
    # the Runge-Kutta warm-up and sample prediction are not fused: the walk refuses, the plan is None, the loop takes _GenericTail
    for skw, evals in ((dict(skip_prk_steps=False), 13), (dict(prediction_type="sample"), 5)):
        sch2 = _scheduler(**skw)
        pipe2 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu2 := PlmsEmulator())), sch2)
        sch2.set_timesteps(4)
        assert pipe2._fused_plan(False, "cpu", sch2.timesteps, None) is None and (sch2.counter, sch2.ets) == (0, [])
        if "prediction_type" in skw:   # (step itself refuses this type: only the plan is checked)
            continue
        c = pipe2(pe, ne, latents=lat0.clone(), **kw)
        assert "plms_update" not in emu2.calls and sch2.step_calls == evals and torch.isfinite(c).all()
    # the scheduler's step takes no eta: a call with eta != 0 keeps the generic path, as for every other scheduler
    sch3 = _scheduler()
    pipe3 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu3 := PlmsEmulator())), sch3)
    d = pipe3(pe, ne, latents=lat0.clone(), eta=0.5, **kw)
    assert "plms_update" not in emu3.calls and sch3.step_calls == 5 and torch.equal(d, a)
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch4 = _scheduler()
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=Dpm2Emulator()), sch4)
    e = old(pe, ne, latents=lat0.clone(), **kw)
    assert sch4.step_calls == 5 and torch.equal(e, a)
