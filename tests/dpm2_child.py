"""Child of tests/test_gpu_dpm2.py: mi355x_sd_dpm2_update on the device against tests/dpm2_bounds.py. Every case of DB.CASES runs
twice, out and the parked sample S each a view inside a canary buffer (the inputs are followed by NaN): the first launch is held to
the float64 bound over every element of out, with S x's bits after stage 1 and untouched by stage 2; the second launch must equal the
first bit for bit. In stage 1 the view of S holds the canary, a NaN pattern, when the launch starts: a kernel that read it would poison
out, one that skipped an element would leave the canary. Then one captured graph holding the single launch, replayed over a stage-1, a
stage-2 and the next stage-1 row from one fixed coefficient buffer with the noise rewritten in place, against direct launches; the
refusals; and an 8-step (15-launch) pipeline run of each class. Prints one JSON line. ``pipeline`` as the only argument: the pipeline
runs alone (the IEEE-half build).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import dpm2_bounds as DB  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests.step_child import _in, _out, capture, launched, main, refusals, replay_rows, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay  # noqa: E402


def _call(lib, x, eu, et, z, S, out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_dpm2_update(x.data_ptr(), eu.data_ptr(), ops._p(et), ops._p(z), S.data_ptr(), out.data_ptr(), coef.data_ptr(),
                                     gs, gr, batch, n, st)


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = DB.inputs(name)
    s = DB.CASES[name]
    batch, n = v["x"].shape
    second = DB.ROW[s["row"]][4] != 0.0
    mis = s.get("misalign")
    eu = _in(v["eu"], int(mis == "eu"))
    et = None if v["et"] is None else _in(v["et"], int(mis == "et"))
    z = None if s.get("null_noise") else _in(v["z"], int(mis == "z"))
    cin = _in(v["coef"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        out, bits, inside = _out(batch * n, int(mis == "out"))
        S, s_bits, s_inside = _out(batch * n, int(mis == "S"))
        if second:   # the state stage 2 reads; stage 1 starts over the canary
            S.copy_(v["S"].reshape(-1))
        before = s_bits.clone()
        if s.get("alias"):   # out = x, as a loop with one latent buffer
            out.copy_(v["x"].reshape(-1))
            xin = out
        else:
            xin = _in(v["x"], int(mis == "x"))
        res["rc"] = launched(name, _call(lib, xin, eu, et, z, S, out, cin, v["gs"], v["gr"], batch, n, st))
        tally(res, bits, inside)
        if second:   # nothing of the buffer changes, inside the view or outside
            res["overwritten"] += int((s_bits != before).sum().item())
        else:
            tally(res, s_bits, s_inside)
        got.append((out.clone(), S.clone()))
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    r = DB.ratios(dev, *got[0])
    res["ratio"], res["state_off"] = r["out"], r["S_off"]
    res["finite"] = bool(torch.isfinite(got[0][0]).all().item())
    res["rerun_off"] = sum(RB.exact_off(a, b) for a, b in zip(got[1], got[0]))
    ptrs = dict(x=xin, eu=eu, et=et, z=z, S=S, out=out)
    res["misaligned"] = sorted(k for k, t in ptrs.items() if t is not None and t.data_ptr() % 16 != 0)
    if name in ("b2 n1024 rescale stage 1", "b2 n512 vectors stage 2", "b2 n512 stage 2 c0 null noise"):   # the wrapper is the same launch
        S2 = torch.full_like(dev["x"], float("nan")) if not second else dev["S"].clone()
        o = ops.dpm2_update(dev["x"], dev["eu"], dev["et"], None if s.get("null_noise") else dev["z"], S2, v["coef"].cuda(), v["gs"],
                            v["gr"])
        res["wrapper_off"] = sum(RB.exact_off(a.reshape(-1), b) for a, b in zip((o, S2), got[0]))
    return res


def run_graph():
    """a loop with fixed pointers (out = x, one S, one noise plane), CFG and guidance_rescale: rows 10, 11, 12 of the DPM2 a
    v-prediction schedule -- stage 1, stage 2 (c != 0), the next stage 1. Direct launches, each reading its row of the table and its
    own noise plane; then ONE captured launch replayed three times with the row and the noise copied into the buffers it reads. S
    starts as NaN both times, and the noise of the stage-1 rows is NaN."""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in DB.inputs("b3 n1023 odd rescale stage 1").items()}
    batch, n = v["x"].shape
    gs, gr = v["gs"], v["gr"]
    table = torch.tensor(DB.ROWS_V[10:13], dtype=torch.float32).cuda()
    nan = lambda: torch.full((batch, n), float("nan"), device="cuda")  # noqa: E731
    zs = [nan(), v["z"].clone(), nan()]
    x, S, direct = v["x"].clone(), nan(), []
    for i in range(3):
        rc = _call(lib, x, v["eu"], v["et"], zs[i], S, x, table[i], gs, gr, batch, n, ops._stream())
        torch.cuda.synchronize()
        direct.append((x.clone(), S.clone()))
    res = {"rc_direct": rc, "finite": bool(all(torch.isfinite(t).all().item() for d in direct for t in d)),
           "stages": [float(table[i, 4].item()) for i in range(3)], "noisy": [bool(table[i, 3].item() != 0.0) for i in range(3)]}
    x, S, z, cur = v["x"].clone(), nan(), nan(), torch.zeros(5, device="cuda")
    g = capture(res, lambda st: _call(lib, x, v["eu"], v["et"], z, S, x, cur, gs, gr, batch, n, st))
    x.copy_(v["x"])   # (the capture launched nothing, but the loop starts from the inputs whatever it did)
    S.copy_(nan())
    res["replay_off"] = replay_rows(g, cur, table, (x, S), direct, before_row=lambda i: z.copy_(zs[i]))
    return res


def _deviations(but, n, x, eu, et, z, S, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "out is noise": but(out=z), "out overlaps noise": but(out=z + 4 * (n - 1)),
            "sample is out": but(S=out), "sample overlaps out": but(S=out + 4 * (n - 1)),
            "sample overlaps out, no rescale": but(S=out - 4, gr=0.0),
            "sample is x": but(S=x), "sample overlaps x": but(S=x + 4 * (n - 1)),
            "sample overlaps eps_uncond": but(S=eu + 4), "sample overlaps eps_text": but(S=et - 4),
            "sample is noise": but(S=z), "sample overlaps noise": but(S=z - 4 * (n - 1)),
            "sample overlaps coef": but(S=coef - 4 * (n - 1)), "sample overlaps coef's end": but(S=coef + 16),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null sample": but(S=None), "null out": but(out=None),
            "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["dpm2"], 16, (0, 1, 2, 4, 6, 8, 10), _deviations)


def run_pipeline(which):
    """the tiny SD config on 2 x 4 x 16 x 16 latents, 8 steps (15 launches) of DPM2 or DPM2 a, CFG, one torch.Generator(device="cuda")
    seed: fused latents against the pipeline's fused_update=False loop run in float64 on the model outputs the fused loop saw (the
    ancestral step handed the float32 draws of its generator, widened), to the accumulated bound. The parked samples and the noise
    planes the bound needs are rebuilt: the planes are redrawn from the seed, every launch is made once more through the wrapper on the
    loop's recorded latents, carrying S, and must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    anc = which == "dpm2a"
    steps, gs, seed = 8, 7.5, 11
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 16, 16)))
    gen = lambda: torch.Generator(device="cuda").manual_seed(seed)  # noqa: E731
    sch = DB.scheduler(which)
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs, g_fused = [], gen()
    kw = dict(num_inference_steps=steps, guidance_scale=gs)
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, latents=lat0.clone(), generator=g_fused,
                                               callback_on_step_end=lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1], **kw)
    torch.cuda.synchronize()
    stepped = sch.step_calls   # (0: the fused loop never called scheduler.step)
    sigma0 = sch.init_noise_sigma
    xs = [lat0 * sigma0] + xs
    with sch.coefficient_walk():
        coef64 = [sch.dpm2_coefficients(t) for t in sch.timesteps]
    launches = len(coef64)
    g2 = gen()
    zs = [torch.randn(lat0.shape, generator=g2, device="cuda", dtype=torch.float32) if anc else None for _ in range(launches)]
    same_state = bool(torch.equal(g_fused.get_state(), g2.get_state()))
    S, Ss, replay_off = torch.full_like(lat0, float("nan")), [], 0
    for i in range(launches):
        Ss.append(S.clone())
        o = ops.dpm2_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), zs[i], S,
                            torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, 0.0)
        replay_off += RB.exact_off(o, xs[i + 1])
    sch64, g64 = DB.scheduler(which, widen=True), gen()
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(pe, ne, latents=lat0.double(), generator=g64,
                                                                               fused_update=False, **kw)
    same_state = same_state and bool(torch.equal(g64.get_state(), g2.get_state()))
    E = DB.accumulated(xs[:-1], Ss, zs, unet.outs, coef64, gs, 0.0, sigma0=sigma0)
    return {"launches": len(unet.outs), "stepped": stepped, "generic_stepped": sch64.step_calls, "replay_off": replay_off,
            "same_generator_state": same_state, "noisy_rows": sum(1 for c in coef64 if c[3] != 0.0),
            "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME, "generic_dtype": str(generic.dtype),
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("DPM2_JSON", [(k, (lambda k=k: run_case(k))) for k in DB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [(f"pipeline {w}", (lambda w=w: run_pipeline(w))) for w in ("dpm2", "dpm2a")])
