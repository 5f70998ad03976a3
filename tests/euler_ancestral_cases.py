"""The EulerAncestralDiscreteScheduler configurations the tests share, and the toy sampling loop (2 x 4 x 8 x 8 latents,
eps = 0.3 xin cos(0.01 t) + 0.1 pat, seed 0, one pre-drawn noise plane per step) that scripts/make_euler_ancestral_golden.py ran
through the reference's own class to write tests/golden/euler_ancestral/<name>.npz."""
import math
import os

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "euler_ancestral")
SHAPE = (2, 4, 8, 8)

CONFIGS = {   # name: (constructor arguments, num_inference_steps, index of the first timestep run: > 0 = img2img after add_noise)
    "ea_sd_default": (dict(SD), 10, 0),
    "ea_v_trailing": (dict(SD, prediction_type="v_prediction", timestep_spacing="trailing"), 10, 0),
    "ea_leading_offset1": (dict(SD, timestep_spacing="leading", steps_offset=1), 10, 0),
    "ea_linear_betas": (dict(), 10, 0),
    "ea_one_step": (dict(SD), 1, 0),
    "ea_img2img": (dict(SD), 10, 3),
}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def draws(steps, first=0):
    """(x0, pat, the start's noise, one noise plane per step RUN) fp32, the same for every scheduler a case is run through"""
    g = torch.Generator().manual_seed(0)
    x0, pat, n0 = (torch.randn(SHAPE, generator=g) for _ in range(3))
    return x0, pat, n0, [torch.randn(SHAPE, generator=g) for _ in range(steps - first)]


def toy_loop(sch, steps, first=0, dtype=torch.float32, wrap=lambda v: v, unwrap=lambda v: v, step=None):
    """-> (end latents, the whole schedule's timesteps, its sigmas, init_noise_sigma, the noise planes [steps run, *SHAPE]);
    wrap / unwrap: torch <-> the scheduler's tensor type; step(sch, eps, t, x, z) -> prev: how z reaches the scheduler (default: the
    ``noise=`` extension of the product class)"""
    if step is None:
        step = lambda s, eps, t, x, z: s.step(eps, t, x, return_dict=False, noise=z)[0]  # noqa: E731
    x0, pat, n0, zs = draws(steps, first)
    sch.set_timesteps(steps)
    ts = list(sch.timesteps)
    sigma0 = float(unwrap(sch.init_noise_sigma))
    if first:
        t0 = float(unwrap(ts[first]))
        x = sch.add_noise(wrap(x0.to(dtype)), wrap(n0.to(dtype)), wrap(torch.tensor([t0] * SHAPE[0], dtype=torch.float32)))
    else:
        x = wrap(x0.to(dtype) * sigma0)
    for t, z in zip(ts[first:], zs):
        xin = unwrap(sch.scale_model_input(x, t))
        eps = 0.3 * xin * math.cos(0.01 * float(unwrap(t))) + 0.1 * pat.to(dtype)
        x = step(sch, wrap(eps), t, x, wrap(z.to(dtype)))
    sig = unwrap(sch.sigmas)
    return (unwrap(x), [float(unwrap(t)) for t in ts], [float(v) for v in torch.as_tensor(sig).reshape(-1)], sigma0,
            torch.stack(zs))
