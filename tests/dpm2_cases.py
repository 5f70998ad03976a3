"""The KDPM2DiscreteScheduler / KDPM2AncestralDiscreteScheduler configurations the tests share, and the toy sampling loop
(2 x 4 x 8 x 8 latents, eps = 0.3 xin cos(0.01 t) + 0.1 pat, seed 0, one pre-drawn noise plane per model evaluation: the loop of
tests/heun_cases.py with the planes of tests/euler_ancestral_cases.py) that scripts/make_dpm2_golden.py ran through the reference's own
classes to write tests/golden/dpm2/<name>.npz. The same six configurations for both classes; the plain class ignores the planes."""
import math
import os

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dpm2")
SHAPE = (2, 4, 8, 8)

_SIX = {   # name: (constructor arguments, num_inference_steps, index of the first timestep run: > 0 = img2img after add_noise)
    "sd_default": (dict(SD), 10, 0),
    "v_trailing": (dict(SD, prediction_type="v_prediction", timestep_spacing="trailing"), 10, 0),
    "leading_offset1": (dict(SD, timestep_spacing="leading", steps_offset=1), 10, 0),
    "karras": (dict(SD, use_karras_sigmas=True), 10, 0),
    "one_step": (dict(SD), 1, 0),
    "img2img": (dict(SD), 10, 4),   # an even index, as StableDiffusionDenoiser.get_timesteps produces (t_start * order)
}
CONFIGS = {f"{prefix}_{k}": (ancestral,) + v for prefix, ancestral in (("dpm2", False), ("dpm2a", True)) for k, v in _SIX.items()}
TABLES = ("sigmas", "sigmas_interpol", "sigmas_up", "sigmas_down")   # what a golden file holds of the schedule, where the class has it


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def draws(evaluations):
    """(x0, pat, the start's noise, one noise plane per model evaluation RUN) fp32, the same for every scheduler a case is run through"""
    g = torch.Generator().manual_seed(0)
    x0, pat, n0 = (torch.randn(SHAPE, generator=g) for _ in range(3))
    return x0, pat, n0, [torch.randn(SHAPE, generator=g) for _ in range(evaluations)]


def toy_loop(sch, steps, first=0, dtype=torch.float32, wrap=lambda v: v, unwrap=lambda v: v, step=None, ancestral=False):
    """-> (end latents, the whole schedule's timesteps, {table: its values} for every table of TABLES the scheduler has,
    init_noise_sigma, the noise planes [evaluations run, *SHAPE]). wrap / unwrap: torch <-> the scheduler's tensor type;
    step(sch, eps, t, x, z) -> prev: how z reaches the scheduler (default: the ``noise=`` extension of the ancestral product class, and
    no noise argument for the plain one). The loop runs the 2 * steps - 1 - first model evaluations from index `first` on."""
    if step is None:
        step = (lambda s, eps, t, x, z: s.step(eps, t, x, return_dict=False, noise=z)[0]) if ancestral else \
            (lambda s, eps, t, x, z: s.step(eps, t, x, return_dict=False)[0])
    sch.set_timesteps(steps)
    ts = list(sch.timesteps)
    assert len(ts) == 2 * steps - 1
    x0, pat, n0, zs = draws(len(ts) - first)
    sigma0 = float(unwrap(sch.init_noise_sigma))
    tables = {k: [float(v) for v in torch.as_tensor(unwrap(getattr(sch, k))).reshape(-1)] for k in TABLES if hasattr(sch, k)}
    if first:
        t0 = float(unwrap(ts[first]))
        x = sch.add_noise(wrap(x0.to(dtype)), wrap(n0.to(dtype)), wrap(torch.tensor([t0] * SHAPE[0], dtype=torch.float32)))
    else:
        x = wrap(x0.to(dtype) * sigma0)
    for t, z in zip(ts[first:], zs):
        xin = unwrap(sch.scale_model_input(x, t))
        eps = 0.3 * xin * math.cos(0.01 * float(unwrap(t))) + 0.1 * pat.to(dtype)
        x = step(sch, wrap(eps), t, x, wrap(z.to(dtype)))
    return unwrap(x), [float(unwrap(t)) for t in ts], tables, sigma0, torch.stack(zs)
