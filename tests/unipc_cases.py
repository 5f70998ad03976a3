"""The UniPCMultistepScheduler configurations the tests share, and the toy sampling loop of tests/reference_cases.py _scheduler_case
(1 x 4 x 8 x 8 latents, eps = 0.3 xin cos(0.01 t) + 0.1 pat, seed 0) that scripts/make_unipc_golden.py ran through the reference's
own class to write tests/golden/unipc/<name>.npz."""
import math
import os

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unipc")

CONFIGS = {   # name: (constructor arguments besides SD, num_inference_steps, index of the first timestep run)
    "unipc_default": (dict(), 10, 0),
    "unipc_order3": (dict(solver_order=3), 10, 0),
    "unipc_bh1_eps": (dict(solver_type="bh1", predict_x0=False), 8, 0),
    "unipc_karras_v": (dict(use_karras_sigmas=True, prediction_type="v_prediction"), 8, 0),
    "unipc_order1": (dict(solver_order=1), 6, 0),
    "unipc_disable_corrector": (dict(disable_corrector=[0, 3]), 8, 0),
    "unipc_order3_no_lower_final": (dict(lower_order_final=False, solver_order=3), 8, 0),
    "unipc_sample": (dict(prediction_type="sample"), 8, 0),
    "unipc_trailing": (dict(timestep_spacing="trailing"), 8, 0),
    "unipc_img2img": (dict(), 10, 2),
    "unipc_order3_bh1_leading": (dict(solver_order=3, solver_type="bh1", timestep_spacing="leading", steps_offset=1), 9, 0),
}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def toy_loop(sch, steps, first=0, dtype=torch.float32, wrap=lambda v: v, unwrap=lambda v: v):
    """-> (end latents, the timesteps of the whole schedule as floats); wrap / unwrap: torch <-> the scheduler's tensor type"""
    g = torch.Generator().manual_seed(0)
    x0, pat = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    sch.set_timesteps(steps)
    x = wrap(x0.to(dtype))
    for t in list(sch.timesteps)[first:]:
        xin = unwrap(sch.scale_model_input(x, t))
        eps = 0.3 * xin * math.cos(0.01 * float(unwrap(t))) + 0.1 * pat.to(dtype)
        x = sch.step(wrap(eps), t, x, return_dict=False)[0]
    return unwrap(x), [float(unwrap(t)) for t in sch.timesteps]
