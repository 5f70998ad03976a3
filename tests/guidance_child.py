"""Child of tests/test_gpu_guidance.py: mi355x_sd_cfg_rescale_axpby on the device against tests/guidance_bounds.py. Every case of
GB.CASES runs twice into views of canary buffers (inputs followed by NaN): the first output is held to the float64 bound over every
element, the second must equal it bit for bit. Then a torch.cuda.graph replayed with two coefficient rows, the refusals, and a
4-step pipeline run. Prints one JSON line.

  python tests/guidance_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import guidance_bounds as GB  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests.step_child import _in, _out, capture, main, refusals, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay  # noqa: E402


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    x, eu, et, coef, gs, gr = GB.inputs(name)
    batch, n = x.shape
    both = _in(torch.cat([eu.reshape(-1), et.reshape(-1)]))   # the two halves of one tensor, as pipeline.py calls it
    cin = _in(coef)
    res = {"unwritten": 0, "overwritten": 0}
    outs = []
    for _ in range(2):
        out, bits, inside = _out(batch * n)
        if GB.CASES[name].get("alias"):   # out = x, as a loop updates its latents in place
            out.copy_(x.reshape(-1))
            xin = out
        else:
            xin = _in(x)
        res["rc"] = lib.mi355x_sd_cfg_rescale_axpby(xin.data_ptr(), both.data_ptr(), both.data_ptr() + 4 * batch * n, out.data_ptr(),
                                                    cin.data_ptr(), gs, gr, batch, n, st)
        torch.cuda.synchronize()
        tally(res, bits, inside)
        outs.append(out.clone())
    xd, ud, td = x.cuda(), eu.cuda(), et.cuda()
    ref, e, _ = GB.cfg_rescale_axpby(xd, ud, td, coef, gs, gr)
    res["ratio"] = RB.check(outs[0].reshape(batch, n), ref, e)
    res["rerun_off"] = RB.exact_off(outs[1], outs[0])
    if gr == 0.0:   # the plain guidance combine, inside that op's own bound
        res["cfg_ratio"] = RB.check(outs[0].reshape(batch, n), *RB.cfg_axpby(xd, ud, td, coef, gs))
    if GB.CASES[name].get("alias") is None and name == "b2 n4096 exact":   # the wrapper is the same launch
        res["wrapper_off"] = RB.exact_off(ops.cfg_rescale_axpby(xd, ud, td, coef.cuda(), gs, gr).reshape(-1), outs[0])
    return res


def run_graph():
    """one capture, two replays with different (a, b) in the device buffer the launch reads"""
    lib = _lib.load()
    x, eu, et, _, gs, gr = (v.cuda() if torch.is_tensor(v) else v for v in GB.inputs("b3 n4092 ragged"))
    batch, n = x.shape
    rows = torch.tensor([GB.COEF, (1.0127, -0.0423)])
    cur, out = torch.zeros(2, device="cuda"), torch.zeros_like(x)
    res = {"unwritten": 0, "overwritten": 0}
    g = capture(res, lambda st: lib.mi355x_sd_cfg_rescale_axpby(x.data_ptr(), eu.data_ptr(), et.data_ptr(), out.data_ptr(), cur.data_ptr(),
                                                                gs, gr, batch, n, st))
    worst = 0.0
    for row in rows:
        cur.copy_(row.cuda())
        g.replay()
        torch.cuda.synchronize()
        ref, e, _ = GB.cfg_rescale_axpby(x, eu, et, row, gs, gr)
        worst = max(worst, RB.check(out, ref, e))
    res["ratio"] = worst
    return res


def _deviations(but, n, x, eu, et, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "per_sample 1": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null": but(eu=None)}


def run_refusals():
    return refusals(FORMS["guidance"], 8, (0, 1, 2, 4, 6), _deviations)


def run_pipeline():
    """the tiny SD config, 4 steps, v-prediction Euler, CFG, guidance_rescale 0.7: fused latents against the generic loop run in
    float64 on the model outputs the fused loop saw, to the accumulated bound"""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import EulerDiscreteScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs, gr = 4, 7.5, 0.7
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 8, 8)))
    sch = EulerDiscreteScheduler(prediction_type="v_prediction", beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs = []
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr,
                                               latents=lat0.clone(),
                                               callback_on_step_end=lambda p, i, t, kw: (xs.append(kw["latents"].clone()), kw)[1])
    torch.cuda.synchronize()
    stepped = sch.step_index   # (None: the fused loop never called scheduler.step)
    sigma0 = float(sch.init_noise_sigma)
    xs = [lat0 * sigma0] + xs
    coef64 = [sch.step_coefficients(t) for t in sch.timesteps]
    sch._step_index = None
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
        pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr, latents=lat0.double(), fused_update=False)
    E = GB.accumulated(xs[:-1], unet.outs, coef64, gs, gr, sigma0)
    return {"steps": len(unet.outs), "stepped": stepped, "finite": bool(torch.isfinite(fused).all().item()),
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("GUIDANCE_JSON", [(k, (lambda k=k: run_case(k))) for k in GB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
