"""Child of tests/test_gpu_singlestep.py: mi355x_sd_singlestep_update on the device against tests/singlestep_bounds.py. Every case of
SB.CASES runs twice, out, the parked sample P and the two planes H each a view inside a canary buffer (the inputs are followed by
NaN, and whatever state the row must not read IS NaN): the first launch is held to the float64 bound over every element of out and of
the plane the row writes; P must be x's bits on an order-1 row; everything else of P and H, inside the views and around them, must
keep its bits; the second launch must equal the first bit for bit. Then one captured graph holding the single launch, replayed over
rows of order 1, 2, 3 and 1 again from one fixed coefficient buffer, against direct launches; the refusals; and a 9-step order-3
pipeline run. Prints one JSON line.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests import singlestep_bounds as SB  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_child import _in, _out, capture, launched, main, refusals, replay_rows, tally  # noqa: E402
from tests.step_pieces import Recording, Replay  # noqa: E402


def _call(lib, x, eu, et, P, H, out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_singlestep_update(x.data_ptr(), eu.data_ptr(), ops._p(et), P.data_ptr(), H.data_ptr(), out.data_ptr(),
                                           coef.data_ptr(), gs, gr, batch, n, st)


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = SB.inputs(name)
    s = SB.CASES[name]
    batch, n = v["x"].shape
    mis = s.get("misalign")
    eu = _in(v["eu"], int(mis == "eu"))
    et = None if v["et"] is None else _in(v["et"], int(mis == "et"))
    cin = _in(v["coef"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        out, bits, inside = _out(batch * n, int(mis == "out"))
        P, pbits, _ = _out(batch * n, int(mis == "P"))
        H, hbits, _ = _out(2 * batch * n, int(mis == "H"))
        P.copy_(v["P"].reshape(-1))   # the state a row may read, NaN wherever it must not; what it writes is compared below
        H.copy_(v["H"].reshape(-1))
        before = (pbits.clone(), hbits.clone())
        if s.get("alias"):   # out = x, as a loop with one latent buffer
            out.copy_(v["x"].reshape(-1))
            xin = out
        else:
            xin = _in(v["x"], int(mis == "x"))
        res["rc"] = launched(name, _call(lib, xin, eu, et, P, H, out, cin, v["gs"], v["gr"], batch, n, st))
        tally(res, bits, inside)
        # around the views of P and H nothing changes (inside them: ratios() below, element by element)
        for b, b0, view in ((pbits, before[0], P), (hbits, before[1], H)):
            outside = torch.ones_like(b, dtype=torch.bool)
            lo = (view.data_ptr() - b.data_ptr()) // 4
            outside[lo:lo + view.numel()] = False
            res["overwritten"] += int(((b != b0) & outside).sum().item())
        got.append((out.clone(), P.clone(), H.clone()))
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    r = SB.ratios(dev, *got[0])
    res["ratio"], res["ratio_hist"], res["state_off"] = r["out"], r["hist"], r["state_off"]
    res["finite"] = bool(torch.isfinite(got[0][0]).all().item())
    res["rerun_off"] = sum(RB.exact_off(a, b) for a, b in zip(got[1], got[0]))
    ptrs = dict(x=xin, eu=eu, et=et, P=P, H=H, out=out)
    res["misaligned"] = sorted(k for k, t in ptrs.items() if t is not None and t.data_ptr() % 16 != 0)
    if name in SB.WRAPPED:   # the wrapper is the same launch
        P2, H2 = dev["P"].clone(), dev["H"].clone()
        o = ops.singlestep_update(dev["x"], dev["eu"], dev["et"], P2, H2, v["coef"].cuda(), v["gs"], v["gr"])
        res["wrapper_off"] = sum(RB.exact_off(a.reshape(-1), b) for a, b in zip((o, P2, H2), got[0]))
    return res


GRAPH_ROWS = ("v_o1", "v_o2k1", "v_o3h", "v_o1")   # park; the group's second output kept; all of the state read; park again


def run_graph():
    """a loop with fixed pointers (out = x, one P, one H), CFG and guidance_rescale over rows of order 1, 2 (keep), 3 (heun) and 1.
    Direct launches, each reading its row of the table; then ONE captured launch replayed four times with the row copied into the
    buffer it reads. P and H start as NaN both times: the first row reads neither, the others only what the rows before them wrote."""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in SB.inputs("b2 n1024 rescale v_o1").items()}
    batch, n = v["x"].shape
    gs, gr = v["gs"], v["gr"]
    table = torch.tensor([SB.ROW[r] for r in GRAPH_ROWS], dtype=torch.float32).cuda()
    nan = lambda *lead: torch.full(lead + (batch, n), float("nan"), device="cuda")  # noqa: E731
    x, P, H, direct = v["x"].clone(), nan(), nan(2), []
    for i in range(len(GRAPH_ROWS)):
        rc = _call(lib, x, v["eu"], v["et"], P, H, x, table[i], gs, gr, batch, n, ops._stream())
        torch.cuda.synchronize()
        direct.append((x.clone(), P.clone(), H.clone()))
    res = {"rc_direct": rc, "finite": bool(all(torch.isfinite(t).all().item() for d in direct[2:] for t in d)),
           "orders": [float(table[i, 6].item()) for i in range(len(GRAPH_ROWS))]}
    x, P, H, cur = v["x"].clone(), nan(), nan(2), torch.zeros(SB.WIDTH, device="cuda")
    g = capture(res, lambda st: _call(lib, x, v["eu"], v["et"], P, H, x, cur, gs, gr, batch, n, st))
    x.copy_(v["x"])   # (the capture launched nothing, but the loop starts from the inputs whatever it did)
    P.copy_(nan())
    H.copy_(nan(2))
    res["replay_off"] = replay_rows(g, cur, table, (x, P, H), direct)
    return res


def _deviations(but, n, x, eu, et, P, H, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "park is out": but(P=out), "park overlaps out": but(P=out + 4 * (n - 1)),
            "park is x": but(P=x), "park overlaps x, no rescale": but(P=x + 4 * (n - 1), gr=0.0),
            "park overlaps eps_text": but(P=et - 4), "park overlaps coef": but(P=coef - 4 * (n - 1)),
            "hist is out": but(H=out), "second plane of hist overlaps out": but(H=out - 4 * (2 * n - 1)),
            "hist is x": but(H=x), "second plane of hist is eps_text": but(H=et - 4 * n),
            "second plane of hist overlaps coef": but(H=coef - 4 * (2 * n - 1)),
            "hist is park": but(H=P), "second plane of hist is park": but(P=H + 4 * n),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0), "batch -1": but(batch=-1),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null park": but(P=None), "null hist": but(H=None),
            "null out": but(out=None), "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["singlestep"], 16, (0, 1, 2, 4, 6, 10, 12), _deviations)   # H: the planes 6, 7


def run_pipeline():
    """the tiny SD config on 2 x 4 x 16 x 16 latents, 9 steps of order 3 (heun: orders 1 2 3 1 2 3 1 2 1), CFG: fused latents
    against the pipeline's fused_update=False loop run in float64 on the model outputs the fused loop saw, to the accumulated bound.
    The state the bound needs is rebuilt: every launch is made once more through the wrapper on the loop's recorded latents,
    carrying P and H, and must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs, skw = 9, 7.5, dict(solver_order=3, solver_type="heun")
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 16, 16)))
    sch = SB.scheduler(**skw)
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs = []
    kw = dict(num_inference_steps=steps, guidance_scale=gs)
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, latents=lat0.clone(),
                                               callback_on_step_end=lambda p, i, t, k: (xs.append(k["latents"].clone()), k)[1], **kw)
    torch.cuda.synchronize()
    stepped = sch.step_calls   # (0: the fused loop never called scheduler.step)
    xs = [lat0 * sch.init_noise_sigma] + xs
    with sch.coefficient_walk():
        coef64 = [sch.singlestep_coefficients(t) for t in sch.timesteps]
    P, H = torch.full_like(lat0, float("nan")), torch.full((2,) + tuple(lat0.shape), float("nan"), device="cuda")
    states, replay_off = [], 0
    for i in range(len(coef64)):
        states.append((P.clone(), H.clone()))
        o = ops.singlestep_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), P, H,
                                  torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, 0.0)
        replay_off += RB.exact_off(o, xs[i + 1])
    sch64 = SB.scheduler(**skw)
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch64)(pe, ne, latents=lat0.double(), fused_update=False, **kw)
    E = SB.accumulated(xs[:-1], states, unet.outs, coef64, gs, 0.0)
    return {"launches": len(unet.outs), "stepped": stepped, "generic_stepped": sch64.step_calls, "replay_off": replay_off,
            "orders": [int(c[6]) for c in coef64], "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME,
            "generic_dtype": str(generic.dtype), "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}


if __name__ == "__main__":
    main("SINGLESTEP_JSON", [(k, (lambda k=k: run_case(k))) for k in SB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
