"""The fused singlestep DPM-Solver step, host side (no GPU): the denoising loop of StableDiffusionDenoiser with
DPMSolverSinglestepScheduler on the emulated device (tests/abi_emulator_singlestep.py). It takes the fused path -- one
mi355x_sd_singlestep_update per model evaluation, scheduler.step never called, the coefficient row advancing by 32 bytes from row 0 at
the first step run, the parked sample, the two planes and the row's stride at fixed addresses -- and ends where the pipeline's own
fused_update=False loop ends when that is run in float64 on the model outputs the fused loop saw, to the bound of
tests/singlestep_bounds.py accumulated over the launches."""
import os
import re

import pytest
import torch

from paddlemix_amd import _lib, ops
from paddlemix_amd import pipeline as PL
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import DPMSolverSinglestepScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import singlestep_bounds as SB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_plms import PlmsEmulator
from tests.abi_emulator_singlestep import SinglestepEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEUN3 = dict(solver_order=3, solver_type="heun")


class _State(SinglestepEmulator):
    """keeps the pointers, the coefficient row, the parked sample and the planes every call was given"""

    def __init__(self):
        super().__init__()
        self.rows, self.ptrs, self.states = [], [], []

    def mi355x_sd_singlestep_update(self, x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream):
        n = batch * per_sample
        self.rows.append(_flat(coef, 8, torch.float32).clone())
        self.ptrs.append((coef, park, hist))
        self.states.append((_flat(park, n, torch.float32).clone(), _flat(hist, 2 * n, torch.float32).clone()))
        return super().mi355x_sd_singlestep_update(x, eu, et, park, hist, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _gen():
    return torch.Generator().manual_seed(7)


def test_the_abi_surface_has_the_entry():
    header = open(os.path.join(ROOT, "include", "mi355x_sd.h")).read()
    assert re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", header).group(1) == str(_lib.ABI_VERSION) and _lib.ABI_VERSION >= 21
    decl = re.search(r"int mi355x_sd_singlestep_update\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["x", "eps_uncond", "eps_text", "park", "hist", "out", "coef", "guidance_scale", "guidance_rescale", "batch",
                     "per_sample", "stream"]
    res, args = _lib.SIGNATURES["mi355x_sd_singlestep_update"]
    assert len(args) == len(names) and callable(ops.singlestep_update)
    tail = PL._SinglestepTail
    assert tail in PL._TAILS and (tail.walk, tail.entry, tail.whole_schedule) == \
        ("singlestep_coefficients", "mi355x_sd_singlestep_update", False)
    assert PL._TAILS.index(tail) < PL._TAILS.index(PL._LinearTail) and hasattr(DPMSolverSinglestepScheduler, "singlestep_coefficients")
    # no other tail's walk is a method of this class: the first match in _TAILS is the singlestep tail
    assert [c for c in PL._TAILS if hasattr(DPMSolverSinglestepScheduler, c.walk)] == [tail]


CASES = {   # name: (scheduler arguments, steps, guidance scale, guidance rescale, img2img strength or None, orders of the rows run)
    "order2": (dict(), 8, 7.5, 0.0, None, [1, 2] * 4),
    "order3_heun": (HEUN3, 9, 7.5, 0.0, None, [1, 2, 3, 1, 2, 3, 1, 2, 1]),
    "order3_midpoint_no_cfg": (dict(solver_order=3), 9, 1.0, 0.0, None, [1, 2, 3, 1, 2, 3, 1, 2, 1]),
    "img2img_listed3": (HEUN3, 9, 7.5, 0.0, 0.8, [1, 1, 2, 3, 1, 2, 1]),          # starts at index 2: listed 3 -> 1
    "img2img_listed2": (HEUN3, 9, 7.5, 0.0, 0.9, [1, 2, 1, 2, 3, 1, 2, 1]),       # starts at index 1: listed 2 -> 1, listed 3 -> 2
    "rescale_v_karras": (dict(HEUN3, prediction_type="v_prediction", use_karras_sigmas=True), 9, 7.5, 0.7, None,
                         [1, 2, 3, 1, 2, 3, 1, 2, 1]),
    "rescale_dpmsolver": (dict(algorithm_type="dpmsolver", solver_type="heun"), 8, 7.5, 0.7, None, [1, 2] * 4),
}


@pytest.mark.parametrize("which", list(CASES))
def test_fused_singlestep_loop_on_the_emulated_device(which):
    skw, steps, gs, gr, strength, orders = CASES[which]
    cfg = gs > 1.0
    pe, ne, lat0 = _loop_inputs()
    sch = SB.scheduler(**skw)
    emu = _State()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    call = dict(latents=lat0.clone()) if strength is None else dict(image=lat0.clone(), strength=strength)
    run = len(orders)
    first = steps - run
    fused = pipe(pe, ne if cfg else None, generator=_gen(), callback_on_step_end=cb, **call, **kw)
    # step never called, the walk left no state
    assert sch.step_calls == 0 and (sch.step_index, sch.sample, sch._last_order) == (None, None, 0)
    assert sch.model_outputs == [None] * sch.config.solver_order
    assert emu.calls.count("singlestep_update") == run == len(unet.outs)                      # one launch per model evaluation
    assert not {"axpby", "cfg_axpby", "cfg_rescale_axpby", "multistep_update", "unipc_update", "ancestral_update", "heun_update",
                "dpm2_update", "plms_update"} & set(emu.calls)
    assert torch.isfinite(fused).all() and torch.equal(xs[-1], fused)
    # the rows the launches read: row i - first of a table over the timesteps the loop RUNS, 32 bytes apart; the state never moves
    with sch.coefficient_walk():
        coef64 = [sch.singlestep_coefficients(t) for t in sch.timesteps[first:]]
    assert [int(c[6]) for c in coef64] == orders
    assert all(torch.equal(r, torch.tensor(c, dtype=torch.float32)) for r, c in zip(emu.rows, coef64))
    assert [p[0] - emu.ptrs[0][0] for p in emu.ptrs] == [32 * k for k in range(run)]
    assert len({p[1:] for p in emu.ptrs}) == 1 and emu.ptrs[0][1] != emu.ptrs[0][2]
    # the pipeline's fused_update=False loop, float64 on the recorded model outputs
    if strength is not None:
        start = pipe.prepare_image_latents(lat0.clone(), sch.timesteps[first:][:1], 2, _gen())
    else:
        start, call = lat0 * sch.init_noise_sigma, dict(latents=lat0.double())
    sch64 = SB.scheduler(**skw)
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    assert generic.dtype == torch.float64 and sch64.step_calls == run and sch64.step_index == steps
    xs = [start] + xs
    states = [(P.reshape(lat0.shape), H.reshape((2,) + tuple(lat0.shape))) for P, H in emu.states]
    E = SB.accumulated(xs[:-1], states, unet.outs, coef64, gs, gr, cfg)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    assert sch.timesteps.tolist() == sch64.timesteps.tolist() and sch.sigmas.tolist() == sch64.sigmas.tolist()
    # and the unmodified float32 generic loop: reported
    if "latents" in call:
        call = dict(latents=lat0.clone())
    plain = StableDiffusionDenoiser(Replay(unet.config, unet.outs, dtype=torch.float32), SB.scheduler(**skw))(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    print(f"{which}: {run} launches, orders {orders}, |fused - generic float64| / accumulated bound {ratio:.3f}; bound / |latent| at "
          f"most {float((E[-1] / generic.abs()).max()):.2e}; |fused - generic float32| / |latent| at most "
          f"{float(((fused - plain).abs() / generic.abs().max()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_singlestep_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=6, guidance_scale=7.5)
    # fused_update=False selects the generic path
    sch, emu = SB.scheduler(**HEUN3), SinglestepEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), fused_update=False, **kw)
    assert "singlestep_update" not in emu.calls and sch.step_calls == 6
    b = pipe(pe, ne, latents=lat0.clone(), **kw)
    assert emu.calls.count("singlestep_update") == 6 and sch.step_calls == 6
    # (a sanity check only: here each loop feeds its own latents to the bf16 UNet, whose operands round at 2^-9; the test above
    # replays the model outputs and holds the fused loop to the float64 bound)
    assert float((a - b).abs().max()) <= 2.0 ** -9 * float(a.abs().max())
    # the plan: a table over the timesteps handed in, no model-input scales, the scheduler left as it was
    sch.set_timesteps(6)
    plan = pipe._fused_plan(False, "cpu", sch.timesteps[2:], None)
    assert isinstance(plan, PL._SinglestepTail) and tuple(plan.coef.shape) == (4, 8) and plan.coef.dtype == torch.float32
    assert plan.scales is None and (sch.step_index, sch.sample, sch.model_outputs) == (None, None, [None] * 3)
    assert plan.coef[:, 6:].tolist() == [[1.0, 0.0], [1.0, 0.0], [2.0, 0.0], [1.0, 0.0]]   # listed 3 1 2 1, from index 2
    # a row that is not finite (two equal sigmas across an order-2 step under heun) and thresholding switched on after
    # construction: the walk refuses, the plan is None, the scheduler is as it was, and the loop takes _GenericTail
    for spoil in ("sigmas", "thresholding"):
        sch2 = SB.scheduler(solver_type="heun")
        pipe2 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu2 := SinglestepEmulator())), sch2)
        sch2.set_timesteps(6)
        if spoil == "sigmas":
            sch2.sigmas[4] = sch2.sigmas[2]
        else:
            sch2.config.thresholding = True
        assert pipe2._fused_plan(False, "cpu", sch2.timesteps, None) is None
        assert (sch2.step_index, sch2.sample, sch2.model_outputs, sch2._last_order) == (None, None, [None, None], 0)
    sch2.config.thresholding = False
    c = pipe2(pe, ne, latents=lat0.clone(), eta=0.5, **kw)   # (eta != 0 keeps the generic path, as for every other scheduler)
    assert "singlestep_update" not in emu2.calls and sch2.step_calls == 6 and torch.isfinite(c).all()
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch4 = SB.scheduler(**HEUN3)
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=PlmsEmulator()), sch4)
    e = old(pe, ne, latents=lat0.clone(), **kw)
    assert sch4.step_calls == 6 and torch.equal(e, a)
