"""Child of tests/test_gpu_heun.py: mi355x_sd_heun_update on the device against tests/heun_bounds.py. Every case of HB.CASES runs
twice, out and the parked planes S / D each a view inside a canary buffer (the inputs are followed by NaN): the first launch is held
to the float64 bound over every element of out and, in stage 1, of D, with S x's bits; stage 2 must leave S and D bit-identical; the
second launch must equal the first bit for bit. In stage 1 the views of S and D hold the canary, a NaN pattern, when the launch
starts: a kernel that read them would poison out, one that skipped an element would leave the canary. Then one captured graph holding
the single launch, replayed over a stage-1, a stage-2 and the next stage-1 row from one fixed coefficient buffer, against direct
launches; the refusals; and an 8-step (15-launch) pipeline run. Prints one JSON line.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import heun_bounds as HB  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests.step_child import _in, _out, capture, launched, main, refusals, replay_rows, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay, counting  # noqa: E402


def _call(lib, x, eu, et, S, D, out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_heun_update(x.data_ptr(), eu.data_ptr(), ops._p(et), S.data_ptr(), D.data_ptr(), out.data_ptr(),
                                     coef.data_ptr(), gs, gr, batch, n, st)


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = HB.inputs(name)
    s = HB.CASES[name]
    batch, n = v["x"].shape
    second = HB.ROW[s["row"]][4] != 0.0
    mis = s.get("misalign")
    eu = _in(v["eu"], int(mis == "eu"))
    et = None if v["et"] is None else _in(v["et"], int(mis == "et"))
    cin = _in(v["coef"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        out, bits, inside = _out(batch * n, int(mis == "out"))
        planes = [_out(batch * n, int(mis == k)) for k in ("S", "D")]
        if second:   # the state stage 2 reads (a NaN D at g == 0 included); stage 1 starts over the canary
            for (view, _, _), k in zip(planes, ("S", "D")):
                view.copy_(v[k].reshape(-1))
        before = [b.clone() for _, b, _ in planes]
        if s.get("alias"):   # out = x, as a loop with one latent buffer
            out.copy_(v["x"].reshape(-1))
            xin = out
        else:
            xin = _in(v["x"], int(mis == "x"))
        S, D = planes[0][0], planes[1][0]
        res["rc"] = launched(name, _call(lib, xin, eu, et, S, D, out, cin, v["gs"], v["gr"], batch, n, st))
        tally(res, bits, inside)
        for (_, b, ins), b0 in zip(planes, before):
            if second:   # nothing of the buffer changes, inside the view or outside
                res["overwritten"] += int((b != b0).sum().item())
            else:
                tally(res, b, ins)
        got.append((out.clone(), S.clone(), D.clone()))
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    r = HB.ratios(dev, *got[0])
    res["ratio"], res["ratio_D"], res["state_off"] = r["out"], r["D"], r["S_off"]
    res["finite"] = bool(torch.isfinite(got[0][0]).all().item())
    res["rerun_off"] = sum(RB.exact_off(a, b) for a, b in zip(got[1], got[0]))
    ptrs = dict(x=xin, eu=eu, et=et, S=S, D=D, out=out)
    res["misaligned"] = sorted(k for k, t in ptrs.items() if t is not None and t.data_ptr() % 16 != 0)
    if name in ("b2 n1024 rescale stage 1", "b2 n512 vectors stage 2"):   # the wrapper is the same launch
        S2, D2 = (torch.full_like(dev["x"], float("nan")) for _ in range(2)) if not second else (dev["S"].clone(), dev["D"].clone())
        o = ops.heun_update(dev["x"], dev["eu"], dev["et"], S2, D2, v["coef"].cuda(), v["gs"], v["gr"])
        res["wrapper_off"] = sum(RB.exact_off(a.reshape(-1), b) for a, b in zip((o, S2, D2), got[0]))
    return res


def run_graph():
    """a loop with fixed pointers (out = x, one S, one D), CFG and guidance_rescale: rows 10, 11, 12 of the v-prediction schedule --
    stage 1, stage 2, the next stage 1. Direct launches, each reading its row of the table; then ONE captured launch replayed three
    times with the row copied into the buffer it reads. S and D start as NaN both times."""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in HB.inputs("b3 n1023 odd rescale stage 1").items()}
    batch, n = v["x"].shape
    gs, gr = v["gs"], v["gr"]
    table = torch.tensor(HB.ROWS_V[10:13], dtype=torch.float32).cuda()
    nan = lambda: torch.full((batch, n), float("nan"), device="cuda")  # noqa: E731
    x, S, D, direct = v["x"].clone(), nan(), nan(), []
    for i in range(3):
        rc = _call(lib, x, v["eu"], v["et"], S, D, x, table[i], gs, gr, batch, n, ops._stream())
        torch.cuda.synchronize()
        direct.append((x.clone(), S.clone(), D.clone()))
    res = {"rc_direct": rc, "finite": bool(all(torch.isfinite(t).all().item() for d in direct for t in d)),
           "stages": [float(table[i, 4].item()) for i in range(3)]}
    x, S, D, cur = v["x"].clone(), nan(), nan(), torch.zeros(5, device="cuda")
    g = capture(res, lambda st: _call(lib, x, v["eu"], v["et"], S, D, x, cur, gs, gr, batch, n, st))
    x.copy_(v["x"])   # (the capture launched nothing, but the loop starts from the inputs whatever it did)
    S.copy_(nan())
    D.copy_(nan())
    res["replay_off"] = replay_rows(g, cur, table, (x, S, D), direct)
    return res


def _deviations(but, n, x, eu, et, S, D, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "sample is out": but(S=out), "sample overlaps out": but(S=out + 4 * (n - 1)),
            "deriv is out": but(D=out), "deriv overlaps out, no rescale": but(D=out - 4, gr=0.0),
            "sample is x": but(S=x), "sample overlaps x": but(S=x + 4 * (n - 1)),
            "deriv is x": but(D=x), "deriv overlaps eps_uncond": but(D=eu + 4),
            "sample overlaps eps_text": but(S=et - 4), "sample overlaps coef": but(S=coef - 4 * (n - 1)),
            "deriv overlaps coef": but(D=coef + 16),
            "sample is deriv": but(S=D), "sample overlaps deriv": but(S=D - 4 * (n - 1)),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null sample": but(S=None), "null deriv": but(D=None),
            "null out": but(out=None), "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["heun"], 16, (0, 1, 2, 4, 6, 8, 10), _deviations)


def run_pipeline():
    """the tiny SD config on 2 x 4 x 16 x 16 latents, 8 steps of Heun (15 launches), CFG: fused latents against the pipeline's
    fused_update=False loop run in float64 on the model outputs the fused loop saw, to the accumulated bound. The parked planes the
    bound needs are rebuilt: every launch is made once more through the wrapper on the loop's recorded latents, carrying S and D, and
    must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import HeunDiscreteScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs = 8, 7.5
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 16, 16)))
    sch = counting(HeunDiscreteScheduler(**HB.SCHED))
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs = []
    kw = dict(num_inference_steps=steps, guidance_scale=gs)
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, latents=lat0.clone(),
                                               callback_on_step_end=lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1], **kw)
    torch.cuda.synchronize()
    stepped = sch.step_calls   # (0: the fused loop never called scheduler.step)
    sigma0 = sch.init_noise_sigma
    xs = [lat0 * sigma0] + xs
    with sch.coefficient_walk():
        coef64 = [sch.heun_coefficients(t) for t in sch.timesteps]
    S, D = (torch.full_like(lat0, float("nan")) for _ in range(2))
    states, replay_off = [], 0
    for i in range(len(coef64)):
        states.append((S.clone(), D.clone()))
        o = ops.heun_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), S, D,
                            torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, 0.0)
        replay_off += RB.exact_off(o, xs[i + 1])
    sch64 = counting(HeunDiscreteScheduler(**HB.SCHED))
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(pe, ne, latents=lat0.double(), fused_update=False, **kw)
    E = HB.accumulated(xs[:-1], states, unet.outs, coef64, gs, 0.0, sigma0=sigma0)
    return {"launches": len(unet.outs), "stepped": stepped, "generic_stepped": sch64.step_calls, "replay_off": replay_off,
            "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME, "generic_dtype": str(generic.dtype),
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("HEUN_JSON", [(k, (lambda k=k: run_case(k))) for k in HB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
