"""Child of tests/test_gpu_ancestral.py: mi355x_sd_ancestral_update on the device against tests/ancestral_bounds.py. Every case of
AB.CASES runs twice into a view inside a canary buffer (inputs followed by NaN): the first launch is held to the float64 bound over
every element, the second must equal the first bit for bit. Then one captured graph holding the single launch, replayed over three
consecutive rows with the noise plane rewritten in place, against three direct launches; the refusals; and an 8-step pipeline run.
Prints one JSON line.

  python tests/ancestral_child.py            every case, the graph, the refusals, the pipeline
  python tests/ancestral_child.py pipeline   the pipeline alone (the build MI355X_SD_DTYPE selects)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import ancestral_bounds as AB  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests.step_child import _in, _out, capture, launched, main, refusals, replay_rows, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay, counting  # noqa: E402

def _call(lib, x, eu, et, z, out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_ancestral_update(x.data_ptr(), eu.data_ptr(), ops._p(et), ops._p(z), out.data_ptr(), coef.data_ptr(), gs, gr,
                                          batch, n, st)


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = AB.inputs(name)
    s = AB.CASES[name]
    batch, n = v["x"].shape
    mis = s.get("misalign")
    eu = _in(v["eu"], int(mis == "eu"))
    et = None if v["et"] is None else _in(v["et"], int(mis == "et"))
    z = None if s.get("null_noise") else _in(v["z"], int(mis == "z"))
    cin = _in(v["coef"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        out, bits, inside = _out(batch * n, int(mis == "out"))
        if s.get("alias"):   # out = x, as a loop with one latent buffer
            out.copy_(v["x"].reshape(-1))
            xin = out
        else:
            xin = _in(v["x"], int(mis == "x"))
        res["rc"] = launched(name, _call(lib, xin, eu, et, z, out, cin, v["gs"], v["gr"], batch, n, st))
        tally(res, bits, inside)
        got.append(out.clone())
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    res["ratio"] = AB.ratio(dev, got[0])
    res["finite"] = bool(torch.isfinite(got[0]).all().item())
    res["rerun_off"] = RB.exact_off(got[1], got[0])
    ptrs = dict(x=xin, eu=eu, et=et, z=z, out=out)
    res["misaligned"] = sorted(k for k, t in ptrs.items() if t is not None and t.data_ptr() % 16 != 0)
    if name == "b2 n1024 rescale":   # the wrapper is the same launch
        o = ops.ancestral_update(dev["x"], dev["eu"], dev["et"], dev["z"], v["coef"].cuda(), v["gs"], v["gr"])
        res["wrapper_off"] = RB.exact_off(o.reshape(-1), got[0])
    return res


def run_graph():
    """a three-step loop with fixed pointers (out = x, one noise plane): the last three rows of the schedule, so the third has c = 0
    and replays over a NaN plane; CFG and guidance_rescale. Three direct launches, each reading its row of the table; then ONE
    captured launch replayed three times with the row and the noise copied into the buffers it reads."""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in AB.inputs("b3 n1023 odd rescale").items()}
    batch, n = v["x"].shape
    gs, gr = v["gs"], v["gr"]
    table = torch.tensor(AB.ROWS_V[-3:], dtype=torch.float32).cuda()
    g0 = torch.Generator(device="cuda").manual_seed(3)
    planes = [torch.randn(batch, n, generator=g0, device="cuda") for _ in range(2)] + [torch.full((batch, n), float("nan"), device="cuda")]
    x, direct = v["x"].clone(), []
    for i in range(3):
        rc = _call(lib, x, v["eu"], v["et"], planes[i], x, table[i], gs, gr, batch, n, ops._stream())
        torch.cuda.synchronize()
        direct.append(x.clone())
    res = {"rc_direct": rc, "finite": bool(torch.isfinite(direct[-1]).all().item()), "last_c": float(table[2, 2].item())}
    x, cur, z = v["x"].clone(), torch.zeros(3, device="cuda"), torch.zeros(batch, n, device="cuda")
    g = capture(res, lambda st: _call(lib, x, v["eu"], v["et"], z, x, cur, gs, gr, batch, n, st))
    x.copy_(v["x"])   # (the capture launched nothing, but the loop starts from the inputs whatever it did)
    res["replay_off"] = replay_rows(g, cur, table, (x,), [(d,) for d in direct], before_row=lambda i: z.copy_(planes[i]))
    return res


def _deviations(but, n, x, eu, et, z, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out overlaps noise": but(out=z + 4 * (n - 1)),
            "out is noise": but(out=z),
            "out overlaps noise, no rescale": but(out=z - 4, gr=0.0),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null out": but(out=None), "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["ancestral"], 12, (0, 1, 2, 3, 5, 7), _deviations)


def run_pipeline():
    """the tiny SD config, 8 steps of Euler a, CFG, guidance_rescale 0.7, one torch.Generator(device="cuda") seed: fused latents against
    the pipeline's fused_update=False loop run in float64 on the model outputs the fused loop saw (its step handed the float32 draws of
    its generator, widened: AB.counting), to the accumulated bound. The noise planes the bound needs are redrawn from the seed: every
    step is launched once more on them and must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import EulerAncestralDiscreteScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs, gr, seed = 8, 7.5, 0.7, 11
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 8, 8)))
    gen = lambda: torch.Generator(device="cuda").manual_seed(seed)  # noqa: E731
    sch = counting(EulerAncestralDiscreteScheduler(**AB.SCHED))
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs, g_fused = [], gen()
    kw = dict(num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr)
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, latents=lat0.clone(), generator=g_fused,
                                               callback_on_step_end=lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1], **kw)
    torch.cuda.synchronize()
    stepped = sch.step_calls   # (0: the fused loop never called scheduler.step)
    sigma0 = sch.init_noise_sigma
    xs = [lat0 * sigma0] + xs
    coef64 = [sch.ancestral_coefficients(t) for t in sch.timesteps]
    sch.set_timesteps(steps)
    g2 = gen()
    zs = [torch.randn(lat0.shape, generator=g2, device="cuda", dtype=torch.float32) for _ in range(steps)]

    def after():   # a generator of the seed after one plane per step, the last step's included
        ga = gen()
        for _ in range(steps):
            torch.randn(lat0.shape, generator=ga, device="cuda", dtype=torch.float32)
        return ga
    same_state = bool(torch.equal(torch.randn(5, generator=g_fused, device="cuda"), torch.randn(5, generator=after(), device="cuda")))
    replay_off = 0
    for i in range(steps):
        o = ops.ancestral_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), zs[i],
                                 torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, gr)
        replay_off += RB.exact_off(o, xs[i + 1])
    sch64, g64 = counting(EulerAncestralDiscreteScheduler(**AB.SCHED), widen=True), gen()
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(pe, ne, latents=lat0.double(), generator=g64,
                                                                               fused_update=False, **kw)
    same_state = same_state and bool(torch.equal(torch.randn(5, generator=g64, device="cuda"), torch.randn(5, generator=after(), device="cuda")))
    E = AB.accumulated(xs[:-1], zs, unet.outs, coef64, gs, gr, sigma0=sigma0)
    return {"steps": len(unet.outs), "stepped": stepped, "generic_stepped": sch64.step_calls, "replay_off": replay_off,
            "same_generator_state": same_state, "last_c": coef64[-1][2],
            "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME,
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("ANCESTRAL_JSON", [(k, (lambda k=k: run_case(k))) for k in AB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
