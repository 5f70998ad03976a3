"""The fused two-stage device step for Heun sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser with
HeunDiscreteScheduler on the emulated device (tests/abi_emulator_heun.py). It takes the fused path -- one mi355x_sd_heun_update per
model evaluation, 2n - 1 of them, scheduler.step never called, the coefficient row advancing by 20 bytes and the parked planes at
fixed addresses -- and ends where the pipeline's own fused_update=False loop ends when that is run in float64 on the model outputs the
fused loop saw, to the bound of tests/heun_bounds.py accumulated over the launches."""
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser, _GenericTail, _HeunTail
from paddlemix_amd.schedulers import HeunDiscreteScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import heun_bounds as HB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_ancestral import AncestralEmulator
from tests.abi_emulator_heun import HeunEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay, counting

STEPS = 8


class _State(HeunEmulator):
    """keeps the pointers, the coefficient row and the parked planes every call was given"""

    def __init__(self):
        super().__init__()
        self.rows, self.ptrs, self.states = [], [], []

    def mi355x_sd_heun_update(self, x, eu, et, sample, deriv, out, coef, gs, gr, batch, per_sample, stream):
        n = batch * per_sample
        self.rows.append(_flat(coef, 5, torch.float32).clone())
        self.ptrs.append((coef, sample, deriv))
        self.states.append((_flat(sample, n, torch.float32).clone(), _flat(deriv, n, torch.float32).clone()))
        return super().mi355x_sd_heun_update(x, eu, et, sample, deriv, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _scheduler(**kw):
    return counting(HeunDiscreteScheduler(**HB.SCHED, **kw))


def _gen():
    return torch.Generator().manual_seed(7)


@pytest.mark.parametrize("which", ["no_cfg", "cfg", "cfg_rescale", "v_prediction", "karras", "img2img"])
def test_fused_heun_loop_on_the_emulated_device(which):
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which in ("cfg_rescale", "v_prediction") else 0.0)
    cfg = gs > 1.0
    skw = dict(prediction_type="v_prediction", timestep_spacing="trailing") if which == "v_prediction" else \
        dict(use_karras_sigmas=True) if which == "karras" else {}
    pe, ne, lat0 = _loop_inputs()
    sch = _scheduler(**skw)
    emu = _State()
    unet = Recording(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu))
    pipe = StableDiffusionDenoiser(unet, sch)
    xs = []
    kw = dict(num_inference_steps=STEPS, guidance_scale=gs, guidance_rescale=gr)
    cb = lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1]  # noqa: E731
    if which == "img2img":   # strength 0.7: int(8 * 0.7) = 5 steps kept, t_start = 3, the loop starts at index 3 * order = 6
        call, first = dict(image=lat0.clone(), strength=0.7), 6
    else:
        call, first = dict(latents=lat0.clone()), 0
    run = 2 * STEPS - 1 - first
    fused = pipe(pe, ne if cfg else None, generator=_gen(), callback_on_step_end=cb, **call, **kw)
    assert sch.step_calls == 0 and sch.step_index is None and sch.state_in_first_order   # step never called, the walk left no state
    assert emu.calls.count("heun_update") == run == len(unet.outs)                        # one launch per model evaluation
    assert not {"axpby", "cfg_axpby", "cfg_rescale_axpby", "multistep_update", "unipc_update", "ancestral_update"} & set(emu.calls)
    assert torch.isfinite(fused).all() and torch.equal(xs[-1], fused)
    # the rows the launches read: row i of the table over the WHOLE schedule, 20 bytes apart; the parked planes never move
    with sch.coefficient_walk():
        coef64 = [sch.heun_coefficients(t) for t in sch.timesteps]
    assert len(coef64) == 2 * STEPS - 1 and [c[4] for c in coef64] == [float(i % 2) for i in range(2 * STEPS - 1)]
    coef64 = coef64[first:]
    assert all(torch.equal(r, torch.tensor(c, dtype=torch.float32)) for r, c in zip(emu.rows, coef64))
    assert [p[0] - emu.ptrs[0][0] for p in emu.ptrs] == [20 * k for k in range(run)]
    assert len({p[1:] for p in emu.ptrs}) == 1 and emu.ptrs[0][1] != emu.ptrs[0][2]
    # the pipeline's fused_update=False loop, float64 on the recorded model outputs
    sigma0 = sch.init_noise_sigma
    if which == "img2img":
        start = pipe.prepare_image_latents(lat0.clone(), sch.timesteps[first:][:1], 2, _gen())
    else:
        start, call = lat0 * sigma0, dict(latents=lat0.double())
    sch64 = _scheduler(**skw)
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    assert generic.dtype == torch.float64 and sch64.step_calls == run
    xs = [start] + xs
    states = [tuple(t.reshape(lat0.shape) for t in s) for s in emu.states]
    E = HB.accumulated(xs[:-1], states, unet.outs, coef64, gs, gr, cfg, sigma0=sigma0 if "latents" in call else 1.0)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    # the scheduler object: its schedule is what the generic run's is, and apart from the step state a generic run advances
    # (the fused loop never steps) nothing differs
    assert sch.timesteps.tolist() == sch64.timesteps.tolist() and sch.sigmas.tolist() == sch64.sigmas.tolist()
    assert sch.num_inference_steps == sch64.num_inference_steps and sch._index_counter == {} and sch.prev_derivative is None
    assert sch64.step_index == 2 * STEPS - 1
    # and the unmodified float32 generic loop: reported
    if "latents" in call:
        call = dict(latents=lat0.clone())
    plain = StableDiffusionDenoiser(Replay(unet.config, unet.outs, dtype=torch.float32), _scheduler(**skw))(
        pe, ne if cfg else None, generator=_gen(), fused_update=False, **call, **kw)
    print(f"{which}: {run} launches, |fused - generic float64| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}; |fused - generic float32| / |latent| at most "
          f"{float(((fused - plain).abs() / generic.abs().max()).max()):.2e}")
    assert ratio < 1.0


def test_routing_around_the_heun_entry():
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=4, guidance_scale=7.5)
    # fused_update=False selects the generic path
    sch, emu = _scheduler(), HeunEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), fused_update=False, **kw)
    assert "heun_update" not in emu.calls and sch.step_calls == 7
    b = pipe(pe, ne, latents=lat0.clone(), **kw)
    assert emu.calls.count("heun_update") == 7 and sch.step_calls == 7
    # (a sanity check only: here each loop feeds its own latents to the bf16 UNet, whose operands round at 2^-9; the test above
    # replays the model outputs and holds the fused loop to the float64 bound)
    assert float((a - b).abs().max()) <= 2.0 ** -9 * float(a.abs().max())
    # the plan: a table over the whole schedule with the model-input scales, the scheduler left as it was
    sch.set_timesteps(4)
    plan = pipe._fused_plan(False, "cpu", sch.timesteps[2:], None)
    assert isinstance(plan, _HeunTail) and tuple(plan.coef.shape) == (7, 5) and plan.coef.dtype == torch.float32
    assert len(plan.scales) == 7 and sch.step_index is None and sch.state_in_first_order
    assert plan.scales == [1.0 / (float(s) ** 2 + 1) ** 0.5 for s in sch.sigmas[:-1]]
    assert plan.coef[:, 4].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0] and plan.coef[:, 3].tolist() == plan.coef[:, 4].tolist()
    # clip_sample is not linear: the walk refuses, the plan is None and the loop takes _GenericTail (scheduler.step clips)
    sch2 = _scheduler(clip_sample=True)
    pipe2 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu2 := HeunEmulator())), sch2)
    sch2.set_timesteps(4)
    assert pipe2._fused_plan(False, "cpu", sch2.timesteps, None) is None and sch2.step_index is None and sch2.state_in_first_order
    c = pipe2(pe, ne, latents=lat0.clone(), **kw)
    assert "heun_update" not in emu2.calls and sch2.step_calls == 7 and torch.isfinite(c).all()
    assert isinstance(_GenericTail(sch2, {}), _GenericTail)
    # the scheduler's step takes no eta: a call with eta != 0 keeps the generic path, as for every other scheduler
    sch3 = _scheduler()
    pipe3 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu3 := HeunEmulator())), sch3)
    d = pipe3(pe, ne, latents=lat0.clone(), eta=0.5, **kw)
    assert "heun_update" not in emu3.calls and sch3.step_calls == 7 and torch.equal(d, a)
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch4 = _scheduler()
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=AncestralEmulator()), sch4)
    e = old(pe, ne, latents=lat0.clone(), **kw)
    assert sch4.step_calls == 7 and torch.equal(e, a)
