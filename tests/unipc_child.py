"""Child of tests/test_gpu_unipc.py: mi355x_sd_unipc_update on the device against tests/unipc_bounds.py. Every case of UB.CASES runs
twice: out is a view of a canary buffer, last and hist are views of canary buffers filled with the case's state, the inputs are followed
by NaN. out, last and history plane 0 of the first launch are held to the float64 bound over every element, the shifted planes to the
bits of the planes they copy; the second launch must equal the first bit for bit. Then one captured graph node replayed over three
consecutive rows against three direct launches, the refusals, and an 8-step pipeline run. Prints one JSON line.

  python tests/unipc_child.py            every case, the graph, the refusals, the pipeline
  python tests/unipc_child.py pipeline   the pipeline alone (the build MI355X_SD_DTYPE selects)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests import unipc_bounds as UB  # noqa: E402
from tests.step_child import _in, _out, capture, main, overwritten, refusals, replay_rows, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay  # noqa: E402


def _call(lib, x, eu, et, last, hist, order, out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_unipc_update(x.data_ptr(), eu.data_ptr(), ops._p(et), last.data_ptr(), hist.data_ptr(), order, out.data_ptr(),
                                      coef.data_ptr(), gs, gr, batch, n, st)


def _state_in(vals):
    """the state values in a view of a canary buffer: (view, bits, mask)"""
    view, bits, inside = _out(vals.numel())
    view.copy_(vals.reshape(-1))
    return view, bits, inside


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = UB.inputs(name)
    s = UB.CASES[name]
    (batch, n), order = v["x"].shape, v["order"]
    eu, cin = _in(v["eu"]), _in(v["coef"])
    et = None if v["et"] is None else _in(v["et"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        out, obits, oin = _out(batch * n)
        last, lbits, lin = _state_in(v["last"].cuda())
        hist, hbits, hin = _state_in(v["hist"].cuda())
        if s.get("alias"):   # out = x, as a loop with one latent buffer
            out.copy_(v["x"].reshape(-1))
            xin = out
        else:
            xin = _in(v["x"], int(bool(s.get("misalign"))))   # (misalign: one element past a 16-byte boundary)
        res["rc"] = _call(lib, xin, eu, et, last, hist, order, out, cin, v["gs"], v["gr"], batch, n, st)
        torch.cuda.synchronize()
        tally(res, obits, oin)
        res["overwritten"] += overwritten(lbits, lin) + overwritten(hbits, hin)
        got.append((out.clone(), last.clone(), hist.clone()))
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    dev["coef"] = v["coef"]
    res["ratio"], res["ratio_last"], res["ratio_plane0"], res["shift_off"] = UB.ratios(dev, *got[0])
    res["rerun_off"] = sum(RB.exact_off(a, b) for a, b in zip(got[1], got[0]))
    res["misaligned"] = int(xin.data_ptr() % 16 != 0)
    if name == "b2 n256 o3 rescale":   # the wrapper is the same launch
        last, hist = dev["last"].clone(), dev["hist"].clone()
        o = ops.unipc_update(dev["x"], dev["eu"], dev["et"], last, hist, v["coef"].cuda(), v["gs"], v["gr"])
        res["wrapper_off"] = sum(RB.exact_off(a.reshape(-1), b) for a, b in zip((o, last, hist), got[0]))
    return res


def run_graph():
    """a three-step loop with fixed pointers (out = x, one last, one hist): the first three rows of a third-order schedule, CFG and
    guidance_rescale. Three direct launches, each reading its row of the table; then ONE captured launch replayed three times with the
    row copied into the buffer it reads. Every step's latents, last and planes must agree bit for bit."""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in UB.inputs("b2 n255 o2 rescale").items()}
    batch, n = v["x"].shape
    order, gs, gr = 3, v["gs"], v["gr"]
    table = torch.tensor(UB.ROWS3[:3], dtype=torch.float32).cuda()

    def fresh():
        return v["x"].clone(), torch.full_like(v["x"], float("nan")), torch.full((order, batch, n), float("nan"), device="cuda")
    x, last, hist = fresh()
    direct = []
    for i in range(3):
        rc = _call(lib, x, v["eu"], v["et"], last, hist, order, x, table[i], gs, gr, batch, n, ops._stream())
        torch.cuda.synchronize()
        direct.append((x.clone(), last.clone(), hist.clone()))
    res = {"rc_direct": rc, "finite": bool(all(torch.isfinite(t).all() for t in direct[-1]))}
    x, last, hist = fresh()
    cur = torch.zeros(12, device="cuda")
    g = capture(res, lambda st: _call(lib, x, v["eu"], v["et"], last, hist, order, x, cur, gs, gr, batch, n, st))
    x.copy_(v["x"])   # (the capture launched nothing, but the loop starts from the inputs whatever it did)
    last.fill_(float("nan"))
    hist.fill_(float("nan"))
    res["replay_off"] = replay_rows(g, cur, table, (x, last, hist), direct)
    return res


def _deviations(but, n, x, eu, et, last, hist, out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out is last": but(out=last),
            "out overlaps the third plane of hist": but(out=hist + 4 * (3 * n - 1)),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "last is x": but(last=x),
            "last overlaps hist": but(last=hist - 4 * (n - 1)),
            "last overlaps eps_text": but(last=et),
            "hist is x": but(hist=x),
            "hist planes reach last": but(hist=last - 4 * 2 * n),
            "hist overlaps coef": but(hist=coef - 4 * (3 * n - 2)),
            "order 0": but(order=0), "order 4": but(order=4),
            "coef not 16-byte aligned": but(coef=coef + 4),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null last": but(last=None), "null hist": but(hist=None),
            "null out": but(out=None), "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["unipc"], 16, (0, 1, 2, 3, 5, 9, 11), _deviations)   # hist: 3 planes, 5 .. 7


def run_pipeline():
    """the tiny SD config, 8 steps of third-order UniPC, CFG, guidance_rescale 0.7: fused latents against the generic loop run in float64
    on the model outputs the fused loop saw, to the accumulated bound. The state the bound needs is the kernel's own last and hist:
    every step is launched once more on the recorded inputs and must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import UniPCMultistepScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs, gr, order = 8, 7.5, 0.7, 3
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 8, 8)))
    sch = UniPCMultistepScheduler(solver_order=order, **UB.SCHED)
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs = []
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr,
                                               latents=lat0.clone(),
                                               callback_on_step_end=lambda p, i, t, kw: (xs.append(kw["latents"].clone()), kw)[1])
    torch.cuda.synchronize()
    stepped = sch.step_index   # (None: the fused loop never called scheduler.step)
    xs = [lat0] + xs
    coef64 = [sch.unipc_coefficients(t) for t in sch.timesteps]
    sch.set_timesteps(steps)
    last, hist = torch.zeros_like(lat0), torch.zeros((order,) + tuple(lat0.shape), device="cuda")
    lasts, hists, replay_off = [], [], 0
    for i in range(steps):
        lasts.append(last.clone())
        hists.append(hist.clone())
        o = ops.unipc_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), last, hist,
                             torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, gr)
        replay_off += RB.exact_off(o, xs[i + 1])
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
        pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr, latents=lat0.double(), fused_update=False)
    E = UB.accumulated(xs[:-1], lasts, hists, unet.outs, coef64, gs, gr, order)
    return {"steps": len(unet.outs), "stepped": stepped, "generic_stepped": sch.step_index, "replay_off": replay_off,
            "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME,
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("UNIPC_JSON", [(k, (lambda k=k: run_case(k))) for k in UB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
