"""The HeunDiscreteScheduler configurations the tests share, and the toy sampling loop (2 x 4 x 8 x 8 latents,
eps = 0.3 xin cos(0.01 t) + 0.1 pat, seed 0: the loop of tests/euler_ancestral_cases.py without noise planes) that
scripts/make_heun_golden.py ran through the reference's own class to write tests/golden/heun/<name>.npz.

Not among the cases, on purpose: a 2-step schedule (one Heun step from sigma ~ 14.6 to 0.03; the reference's own float32-against-float64
difference is 7e-6 there) and an odd start index (the reference itself runs off its sigma table and returns NaN)."""
import math
import os

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heun")
SHAPE = (2, 4, 8, 8)

CONFIGS = {   # name: (constructor arguments, num_inference_steps, index of the first timestep run: > 0 = img2img after add_noise)
    "heun_sd_default": (dict(SD), 10, 0),
    "heun_v_trailing": (dict(SD, prediction_type="v_prediction", timestep_spacing="trailing"), 10, 0),
    "heun_karras": (dict(SD, use_karras_sigmas=True), 10, 0),
    "heun_leading_offset1": (dict(SD, timestep_spacing="leading", steps_offset=1), 10, 0),
    "heun_one_step": (dict(SD), 1, 0),
    "heun_img2img": (dict(SD), 10, 4),   # an even index, as StableDiffusionDenoiser.get_timesteps produces (t_start * order)
}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def draws():
    """(x0, pat, the start's noise) fp32, the same for every scheduler a case is run through"""
    g = torch.Generator().manual_seed(0)
    return tuple(torch.randn(SHAPE, generator=g) for _ in range(3))


def toy_loop(sch, steps, first=0, dtype=torch.float32, wrap=lambda v: v, unwrap=lambda v: v):
    """-> (end latents, the whole schedule's timesteps, its sigmas, init_noise_sigma); wrap / unwrap: torch <-> the scheduler's
    tensor type. The loop runs the 2 * steps - 1 - first model evaluations from index `first` on."""
    x0, pat, n0 = draws()
    sch.set_timesteps(steps)
    ts = list(sch.timesteps)
    assert len(ts) == 2 * steps - 1
    sigma0 = float(unwrap(sch.init_noise_sigma))
    if first:
        t0 = float(unwrap(ts[first]))
        x = sch.add_noise(wrap(x0.to(dtype)), wrap(n0.to(dtype)), wrap(torch.tensor([t0] * SHAPE[0], dtype=torch.float32)))
    else:
        x = wrap(x0.to(dtype) * sigma0)
    for t in ts[first:]:
        xin = unwrap(sch.scale_model_input(x, t))
        eps = 0.3 * xin * math.cos(0.01 * float(unwrap(t))) + 0.1 * pat.to(dtype)
        x = sch.step(wrap(eps), t, x, return_dict=False)[0]
    sig = unwrap(sch.sigmas)
    return unwrap(x), [float(unwrap(t)) for t in ts], [float(v) for v in torch.as_tensor(sig).reshape(-1)], sigma0
