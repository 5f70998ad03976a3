"""The DPMSolverSinglestepScheduler configurations the tests share, and the toy sampling loop (2 x 4 x 8 x 8 latents,
eps = 0.3 xin cos(0.01 t) + 0.1 pat, seed 0: the loop of tests/dpm2_cases.py without its noise planes) that
scripts/make_singlestep_golden.py ran through the reference's own class to write tests/golden/singlestep/<name>.npz."""
import math
import os

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "singlestep")
SHAPE = (2, 4, 8, 8)

CONFIGS = {   # name: (constructor arguments, num_inference_steps, index of the first timestep run: > 0 = img2img after add_noise)
    "order2_default": (dict(SD), 10, 0),
    "order2_odd": (dict(SD), 7, 0),                                                       # 1 2 1 2 1 2 1
    "order3_heun": (dict(SD, solver_order=3, solver_type="heun"), 10, 0),                 # 1 2 3 1 2 3 1 2 3 1
    "order3_midpoint": (dict(SD, solver_order=3), 9, 0),                                  # 1 2 3 1 2 3 1 2 1
    "order3_no_lower_final": (dict(SD, solver_order=3, solver_type="heun", lower_order_final=False), 9, 0),   # 1 2 3 x 3
    "order3_uneven_no_lower_final": (dict(SD, solver_order=3, lower_order_final=False), 8, 0),   # set_timesteps switches it on
    "dpmsolver_heun_sample": (dict(SD, algorithm_type="dpmsolver", solver_type="heun", prediction_type="sample"), 8, 0),
    "dpmsolver_order3_heun": (dict(SD, algorithm_type="dpmsolver", solver_order=3, solver_type="heun"), 9, 0),
    "karras_v": (dict(SD, use_karras_sigmas=True, prediction_type="v_prediction"), 10, 0),
    "order1": (dict(SD, solver_order=1), 6, 0),
    "one_step": (dict(SD), 1, 0),
    "linear_betas_order3": (dict(solver_order=3, solver_type="heun"), 6, 0),
    "img2img_listed2": (dict(SD, solver_order=3, solver_type="heun"), 10, 4),   # listed 2 -> 1, then listed 3 -> 2
    "img2img_listed3": (dict(SD, solver_order=3, solver_type="heun"), 10, 2),   # listed 3 -> 1
    "img2img_order2": (dict(SD), 10, 3),                                         # listed 2 -> 1
}


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def toy_loop(sch, steps, first=0, dtype=torch.float32, wrap=lambda v: v, unwrap=lambda v: v, seen=None):
    """-> (end latents, the whole schedule's timesteps, its sigmas, its order list). wrap / unwrap: torch <-> the scheduler's tensor
    type. seen: a list that gets (x, eps) of every evaluation, as torch tensors"""
    g = torch.Generator().manual_seed(0)
    x0, pat, n0 = (torch.randn(SHAPE, generator=g) for _ in range(3))
    sch.set_timesteps(steps)
    ts = list(sch.timesteps)
    sigmas = [float(v) for v in torch.as_tensor(unwrap(sch.sigmas)).reshape(-1)]
    if first:
        t0 = int(unwrap(ts[first]))
        x = sch.add_noise(wrap(x0.to(dtype)), wrap(n0.to(dtype)), wrap(torch.tensor([t0] * SHAPE[0], dtype=torch.int64)))
    else:
        x = wrap(x0.to(dtype) * float(unwrap(sch.init_noise_sigma)))
    for t in ts[first:]:
        xin = unwrap(sch.scale_model_input(x, t))
        eps = 0.3 * xin * math.cos(0.01 * float(unwrap(t))) + 0.1 * pat.to(dtype)
        if seen is not None:
            seen.append((unwrap(x).clone(), eps.clone()))
        x = sch.step(wrap(eps), t, x, return_dict=False)[0]
    return unwrap(x), [float(unwrap(t)) for t in ts], sigmas, [int(o) for o in sch.order_list]
