"""The PNDMScheduler (skip_prk_steps: PLMS) configurations the PLMS tests share, and the toy sampling loop of tests/heun_cases.py
(2 x 4 x 8 x 8 latents, eps = 0.3 x cos(0.01 t) + 0.1 pat, seed 0) run through ``scheduler.step`` with every (x, e) pair recorded.

The class itself is pinned against the reference elsewhere (tests/test_schedulers.py, sched_pndm_* of tests/reference_cases.py); these
cases are for ``plms_coefficients``, which must say what ``step`` does: n steps are n + 1 evaluations (the second timestep is visited
twice; ``set_timesteps(1)`` has no second one and gives a single evaluation), and 1, 2 and 3 steps end a loop on each of the shorter
history branches."""
import math

import torch

from tests.heun_cases import SD, SHAPE, draws

PLMS = dict(SD, skip_prk_steps=True)

CONFIGS = {   # name: (constructor arguments, num_inference_steps, index of the first timestep run: > 0 = img2img after add_noise)
    "plms_sd_default": (dict(PLMS, steps_offset=1), 10, 0),   # what the SD-1.x checkpoints ship (set_alpha_to_one=False)
    "plms_v_trailing": (dict(PLMS, prediction_type="v_prediction", timestep_spacing="trailing"), 10, 0),
    "plms_linspace": (dict(PLMS, timestep_spacing="linspace"), 10, 0),
    "plms_alpha_to_one": (dict(PLMS, set_alpha_to_one=True), 10, 0),   # steps_offset = 0: the last t_prev is negative
    "plms_one_step": (dict(PLMS, steps_offset=1), 1, 0),       # 1 evaluation: the parking row alone
    "plms_two_steps": (dict(PLMS, steps_offset=1), 2, 0),      # 3: ends on the two-term row
    "plms_three_steps": (dict(PLMS, steps_offset=1), 3, 0),    # 4: ends on the three-term row
    "plms_img2img": (dict(PLMS, steps_offset=1), 10, 4),       # 7 evaluations from inside the schedule, counter starting at 0
}


def toy_loop(sch, steps, first=0, dtype=torch.float64):
    """-> (the latents before every evaluation and after the last one, the model outputs, the timesteps run): the loop runs
    ``sch.timesteps[first:]`` through ``sch.step`` in `dtype`"""
    x0, pat, n0 = draws()
    sch.set_timesteps(steps)
    ts = [int(t) for t in sch.timesteps][first:]
    if first:
        x = sch.add_noise(x0.to(dtype), n0.to(dtype), torch.tensor([ts[0]] * SHAPE[0]))
    else:
        x = x0.to(dtype) * sch.init_noise_sigma
    xs, es = [x], []
    for t in ts:
        e = 0.3 * x * math.cos(0.01 * t) + 0.1 * pat.to(dtype)
        x = sch.step(e, t, x, return_dict=False)[0]
        es.append(e)
        xs.append(x)
    return xs, es, ts
