"""The fused two-stage midpoint step for DPM2 / DPM2 a sampling, host side (no GPU): the denoising loop of StableDiffusionDenoiser
with KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler on the emulated device (tests/abi_emulator_dpm2.py). It takes the
fused path -- one mi355x_sd_dpm2_update per model evaluation, 2n - 1 of them, scheduler.step never called, the coefficient row
advancing by 20 bytes and the parked sample (and, for DPM2 a, the noise) at a fixed address -- and ends where the pipeline's own
fused_update=False loop ends when that is run in float64 on the model outputs the fused loop saw, to the bound of tests/dpm2_bounds.py
accumulated over the launches. For DPM2 a both paths run under one seed and leave the generator in the same state."""
import pytest
import torch

from paddlemix_amd.pipeline import StableDiffusionDenoiser, _Dpm2Tail
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import dpm2_bounds as DB
from tests.abi_emulator import _flat, on_emulator
from tests.abi_emulator_dpm2 import Dpm2Emulator
from tests.abi_emulator_heun import HeunEmulator
from tests.configs import TINY
from tests.step_pieces import Recording, Replay

STEPS, SEED = 8, 7
BOTH = pytest.mark.parametrize("sampler", ["dpm2", "dpm2a"])


class _State(Dpm2Emulator):
    """keeps the pointers, the coefficient row, the parked sample and the noise plane every call was given"""

    def __init__(self):
        super().__init__()
        self.rows, self.ptrs, self.Ss, self.zs = [], [], [], []

    def mi355x_sd_dpm2_update(self, x, eu, et, noise, sample, out, coef, gs, gr, batch, per_sample, stream):
        n = batch * per_sample
        self.rows.append(_flat(coef, 5, torch.float32).clone())
        self.ptrs.append((coef, sample, noise))
        self.Ss.append(_flat(sample, n, torch.float32).clone())
        self.zs.append(_flat(noise, n, torch.float32).clone() if noise else None)
        return super().mi355x_sd_dpm2_update(x, eu, et, noise, sample, out, coef, gs, gr, batch, per_sample, stream)


def _loop_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(2, 7, 64, generator=g), torch.randn(2, 7, 64, generator=g), torch.randn(2, 4, 8, 8, generator=g)


def _gen():
    return torch.Generator().manual_seed(SEED)


@BOTH
@pytest.mark.parametrize("which", ["no_cfg", "cfg", "cfg_rescale", "v_prediction", "karras", "img2img"])
def test_fused_dpm2_loop_on_the_emulated_device(sampler, which):
    anc = sampler == "dpm2a"
    gs, gr = (1.0 if which == "no_cfg" else 7.5), (0.7 if which in ("cfg_rescale", "v_prediction") else 0.0)
    cfg = gs > 1.0
    skw = dict(prediction_type="v_prediction", timestep_spacing="trailing") if which == "v_prediction" else \
        dict(use_karras_sigmas=True) if which == "karras" else {}
    pe, ne, lat0 = _loop_inputs()
    sch = DB.scheduler(sampler, **skw)
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
    g_fused = _gen()
    fused = pipe(pe, ne if cfg else None, generator=g_fused, callback_on_step_end=cb, **call, **kw)
    assert sch.step_calls == 0 and sch.step_index is None and sch.state_in_first_order   # step never called, the walk left no state
    assert emu.calls.count("dpm2_update") == run == len(unet.outs)                        # one launch per model evaluation
    assert not {"axpby", "cfg_axpby", "cfg_rescale_axpby", "multistep_update", "unipc_update", "ancestral_update", "heun_update"} \
        & set(emu.calls)
    assert torch.isfinite(fused).all() and torch.equal(xs[-1], fused)
    # the rows the launches read: row i of the table over the WHOLE schedule, 20 bytes apart; the parked sample and the noise never move
    with sch.coefficient_walk():
        coef64 = [sch.dpm2_coefficients(t) for t in sch.timesteps]
    assert len(coef64) == 2 * STEPS - 1 and [c[4] for c in coef64] == [float(i % 2) for i in range(2 * STEPS - 1)]
    assert all((c[3] > 0.0) == (anc and c[4] == 1.0) for c in coef64)
    coef64 = coef64[first:]
    assert all(torch.equal(r, torch.tensor(c, dtype=torch.float32)) for r, c in zip(emu.rows, coef64))
    assert [p[0] - emu.ptrs[0][0] for p in emu.ptrs] == [20 * k for k in range(run)]
    assert len({p[1:] for p in emu.ptrs}) == 1 and bool(emu.ptrs[0][2]) == anc and emu.ptrs[0][1] != emu.ptrs[0][2]
    # the planes: the generator's draws after whatever the start took, in order, one per evaluation; DPM2 draws nothing
    g = _gen()
    sigma0 = sch.init_noise_sigma
    if which == "img2img":
        start = pipe.prepare_image_latents(lat0.clone(), sch.timesteps[first:][:1], 2, g)
    else:
        start = lat0 * sigma0
    zs = [torch.randn(lat0.shape, generator=g) if anc else None for _ in range(run)]
    if anc:
        assert all(torch.equal(a.reshape(lat0.shape), b) for a, b in zip(emu.zs, zs))
    after = g.get_state()
    assert torch.equal(g_fused.get_state(), after)
    # the pipeline's fused_update=False loop, float64 on the recorded model outputs, the same seed
    sch64 = DB.scheduler(sampler, widen=True, **skw)
    if "latents" in call:
        call = dict(latents=lat0.double())
    g64 = _gen()
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(
        pe, ne if cfg else None, generator=g64, fused_update=False, **call, **kw)
    assert generic.dtype == torch.float64 and sch64.step_calls == run and torch.equal(g64.get_state(), after)
    xs = [start] + xs
    Ss = [s.reshape(lat0.shape) for s in emu.Ss]
    E = DB.accumulated(xs[:-1], Ss, zs, unet.outs, coef64, gs, gr, cfg, sigma0=sigma0 if "latents" in call else 1.0)
    ratio = ((fused.double() - generic).abs() / E[-1]).max().item()
    # the scheduler object: its schedule is what the generic run's is, and apart from the step state a generic run advances
    # (the fused loop never steps) nothing differs
    assert sch.timesteps.tolist() == sch64.timesteps.tolist() and sch.sigmas.tolist() == sch64.sigmas.tolist()
    assert sch.num_inference_steps == sch64.num_inference_steps and sch._index_counter == {} and sch.sample is None
    assert sch64.step_index == 2 * STEPS - 1
    # and the unmodified float32 generic loop: reported, and it leaves the generator where the fused loop left it
    if "latents" in call:
        call = dict(latents=lat0.clone())
    g32 = _gen()
    plain = StableDiffusionDenoiser(Replay(unet.config, unet.outs, dtype=torch.float32), DB.scheduler(sampler, **skw))(
        pe, ne if cfg else None, generator=g32, fused_update=False, **call, **kw)
    assert torch.equal(g32.get_state(), after)
    print(f"{sampler} {which}: {run} launches, |fused - generic float64| / accumulated bound {ratio:.3f}; bound / |latent| at most "
          f"{float((E[-1] / generic.abs()).max()):.2e}; |fused - generic float32| / |latent| at most "
          f"{float(((fused - plain).abs() / generic.abs().max()).max()):.2e}")
    assert ratio < 1.0


@BOTH
def test_routing_around_the_dpm2_entry(sampler):
    anc = sampler == "dpm2a"
    pe, ne, lat0 = _loop_inputs()
    P = synth_unet_params(TINY, seed=1234)
    kw = dict(num_inference_steps=4, guidance_scale=7.5)
    # fused_update=False selects the generic path
    sch, emu = DB.scheduler(sampler), Dpm2Emulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), sch)
    a = pipe(pe, ne, latents=lat0.clone(), generator=_gen(), fused_update=False, **kw)
    assert "dpm2_update" not in emu.calls and sch.step_calls == 7
    b = pipe(pe, ne, latents=lat0.clone(), generator=_gen(), **kw)
    assert emu.calls.count("dpm2_update") == 7 and sch.step_calls == 7
    # (a sanity check only: here each loop feeds its own latents to the bf16 UNet, whose operands round at 2^-9; the test above
    # replays the model outputs and holds the fused loop to the float64 bound)
    assert float((a - b).abs().max()) <= 2.0 ** -9 * float(a.abs().max())
    # the plan: a table over the whole schedule with the model-input scales, the scheduler left as it was
    sch.set_timesteps(4)
    plan = pipe._fused_plan(False, "cpu", sch.timesteps[2:], None)
    assert isinstance(plan, _Dpm2Tail) and tuple(plan.coef.shape) == (7, 5) and plan.coef.dtype == torch.float32 and plan.noisy == anc
    assert len(plan.scales) == 7 and sch.step_index is None and sch.state_in_first_order
    sig = [float(sch.sigmas[i]) if i % 2 == 0 else float(sch.sigmas_interpol[i - 1 if anc else i]) for i in range(7)]
    assert plan.scales == [1.0 / (s ** 2 + 1) ** 0.5 for s in sig]       # sigma_interpol on the second-stage indices
    assert plan.coef[:, 4].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    assert [c > 0.0 for c in plan.coef[:, 3].tolist()] == [anc and i % 2 == 1 for i in range(7)]
    # sample prediction has no row: the walk refuses, the plan is None, and the generic loop raises where the reference does
    sch2 = DB.scheduler(sampler, prediction_type="sample")
    pipe2 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu2 := Dpm2Emulator())), sch2)
    sch2.set_timesteps(4)
    assert pipe2._fused_plan(False, "cpu", sch2.timesteps, None) is None and sch2.step_index is None and sch2.state_in_first_order
    with pytest.raises(NotImplementedError, match="prediction_type not implemented yet: sample"):
        pipe2(pe, ne, latents=lat0.clone(), **kw)
    assert "dpm2_update" not in emu2.calls
    # the scheduler's step takes no eta: a call with eta != 0 keeps the generic path, as for every other scheduler
    sch3 = DB.scheduler(sampler)
    pipe3 = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=(emu3 := Dpm2Emulator())), sch3)
    d = pipe3(pe, ne, latents=lat0.clone(), generator=_gen(), eta=0.5, **kw)
    assert "dpm2_update" not in emu3.calls and sch3.step_calls == 7 and torch.equal(d, a)
    # a test backend from before the entry existed keeps the generic path (the library itself is refused at load on an ABI mismatch)
    sch4 = DB.scheduler(sampler)
    old = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=HeunEmulator()), sch4)
    e = old(pe, ne, latents=lat0.clone(), generator=_gen(), **kw)
    assert sch4.step_calls == 7 and torch.equal(e, a)
