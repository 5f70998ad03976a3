"""Child of tests/test_gpu_multistep.py: mi355x_sd_multistep_update on the device against tests/multistep_bounds.py. Every case of
MB.CASES runs twice into views of canary buffers (inputs followed by NaN): both outputs of the first launch are held to the float64
bound over every element, the second launch must equal the first bit for bit. Then a torch.cuda.graph replayed with two coefficient
rows (D != 0 and D = 0), the refusals, and a 6-step pipeline run. Prints one JSON line.

  python tests/multistep_child.py            every case, the graph, the refusals, the pipeline
  python tests/multistep_child.py pipeline   the pipeline alone (the build MI355X_SD_DTYPE selects)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import multistep_bounds as MB  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests.step_child import _in, _out, capture, main, refusals, tally  # noqa: E402
from tests.step_forms import FORMS  # noqa: E402
from tests.step_pieces import Recording, Replay  # noqa: E402


def _call(lib, x, eu, et, m1, out, m_out, coef, gs, gr, batch, n, st):
    return lib.mi355x_sd_multistep_update(x.data_ptr(), eu.data_ptr(), ops._p(et), m1.data_ptr(), out.data_ptr(), m_out.data_ptr(),
                                          coef.data_ptr(), gs, gr, batch, n, st)


def run_case(name):
    lib, st = _lib.load(), ops._stream()
    v = MB.inputs(name)
    s = MB.CASES[name]
    batch, n = v["x"].shape
    eu, cin = _in(v["eu"]), _in(v["coef"])
    et = None if v["et"] is None else _in(v["et"])
    res = {"unwritten": 0, "overwritten": 0}
    got = []
    for _ in range(2):
        (out, obits, oin), (m_out, mbits, min_) = _out(batch * n), _out(batch * n)
        if s.get("alias"):   # out = x and m_out = m_prev, as a loop with one latent and one history buffer
            out.copy_(v["x"].reshape(-1))
            m_out.copy_(v["m1"].reshape(-1))
            xin, m1 = out, m_out
        else:
            xin, m1 = _in(v["x"], int(bool(s.get("misalign")))), _in(v["m1"])   # (misalign: x one element past a 16-byte boundary)
        res["rc"] = _call(lib, xin, eu, et, m1, out, m_out, cin, v["gs"], v["gr"], batch, n, st)
        torch.cuda.synchronize()
        tally(res, obits, oin)
        tally(res, mbits, min_)
        got.append((out.clone(), m_out.clone()))
    dev = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in v.items()}
    r = MB.multistep_update(dev["x"], dev["eu"], dev["et"], dev["m1"], v["coef"], v["gs"], v["gr"])
    res["ratio"] = RB.check(got[0][0].reshape(batch, n), r["out"], r["e_out"])
    res["ratio_m"] = RB.check(got[0][1].reshape(batch, n), r["m0"], r["e_m0"])
    res["rerun_off"] = RB.exact_off(got[1][0], got[0][0]) + RB.exact_off(got[1][1], got[0][1])
    res["misaligned"] = int(xin.data_ptr() % 16 != 0)
    if name == "b2 n4096 exact":   # the wrapper is the same launch
        o, m = ops.multistep_update(dev["x"], dev["eu"], dev["et"], dev["m1"], v["coef"].cuda(), v["gs"], v["gr"])
        res["wrapper_off"] = RB.exact_off(o.reshape(-1), got[0][0]) + RB.exact_off(m.reshape(-1), got[0][1])
    return res


def run_graph():
    """one capture, two replays with different rows in the device buffer the launch reads: second order, then first order"""
    lib = _lib.load()
    v = {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in MB.inputs("b3 n4093 odd rescale").items()}
    batch, n = v["x"].shape
    cur, out, m_out = torch.zeros(5, device="cuda"), torch.zeros_like(v["x"]), torch.zeros_like(v["x"])
    res = {}
    g = capture(res, lambda st: _call(lib, v["x"], v["eu"], v["et"], v["m1"], out, m_out, cur, v["gs"], v["gr"], batch, n, st))
    worst = 0.0
    for row in (MB.MID, MB.FIRST):
        row = torch.tensor(row, dtype=torch.float32)
        cur.copy_(row.cuda())
        g.replay()
        torch.cuda.synchronize()
        r = MB.multistep_update(v["x"], v["eu"], v["et"], v["m1"], row, v["gs"], v["gr"])
        worst = max(worst, RB.check(out, r["out"], r["e_out"]), RB.check(m_out, r["m0"], r["e_m0"]))
    res["ratio"] = worst
    return res


def _deviations(but, n, x, eu, et, m1, out, m_out, coef):
    return {"out overlaps eps_text": but(out=et + 4 * (n - 1)),
            "out overlaps eps_uncond": but(out=eu - 4),
            "out overlaps x partly": but(out=x + 4, n=n // 2),
            "out overlaps m_prev": but(out=m1),
            "out overlaps m_out": but(out=m_out + 4 * (n - 1)),
            "out is m_out": but(out=m_out),
            "m_out overlaps x": but(m_out=x),
            "m_out overlaps m_prev partly": but(m_out=m1 + 4, n=n // 2),
            "m_out overlaps eps_text": but(m_out=et),
            "out overlaps coef": but(out=coef - 4 * (n - 1)),
            "per_sample 0": but(n=0),
            "per_sample 1 with rescale": but(batch=n, n=1),
            "batch 0": but(batch=0),
            "null x": but(x=None), "null eps_uncond": but(eu=None), "null m_prev": but(m1=None), "null out": but(out=None),
            "null m_out": but(m_out=None), "null coef": but(coef=None)}


def run_refusals():
    return refusals(FORMS["multistep"], 12, (0, 1, 2, 3, 5, 7, 9), _deviations)


def run_pipeline():
    """the tiny SD config, 6 steps of dpmsolver++ 2M, CFG, guidance_rescale 0.7: fused latents against the generic loop run in float64
    on the model outputs the fused loop saw, to the accumulated bound. The history the bound needs is the kernel's own m_out: every
    step is launched once more on the recorded inputs and must reproduce the loop's latents bit for bit."""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import DPMSolverMultistepScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.configs import TINY
    steps, gs, gr = 6, 7.5, 0.7
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = (torch.randn(s, generator=g).cuda() for s in ((2, 7, 64), (2, 7, 64), (2, 4, 8, 8)))
    sch = DPMSolverMultistepScheduler(**MB.SCHED)
    unet = Recording(UNet2DConditionModel(TINY, synth_unet_params(TINY, seed=1234), device="cuda:0"))
    xs = []
    fused = StableDiffusionDenoiser(unet, sch)(pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr,
                                               latents=lat0.clone(),
                                               callback_on_step_end=lambda p, i, t, kw: (xs.append(kw["latents"].clone()), kw)[1])
    torch.cuda.synchronize()
    stepped = sch.step_index   # (None: the fused loop never called scheduler.step)
    xs = [lat0] + xs
    coef64 = [sch.multistep_coefficients(t) for t in sch.timesteps]
    sch.set_timesteps(steps)
    hs, replay_off = [torch.zeros_like(lat0)], 0
    for i in range(steps):
        o, m = ops.multistep_update(xs[i], unet.outs[i][:2].contiguous(), unet.outs[i][2:].contiguous(), hs[i],
                                    torch.tensor(coef64[i], dtype=torch.float32).cuda(), gs, gr)
        replay_off += RB.exact_off(o, xs[i + 1])
        hs.append(m)
    generic = StableDiffusionDenoiser(Replay(unet.config, unet.outs), sch)(
        pe, ne, num_inference_steps=steps, guidance_scale=gs, guidance_rescale=gr, latents=lat0.double(), fused_update=False)
    E = MB.accumulated(xs[:-1], hs[:-1], unet.outs, coef64, gs, gr)
    return {"steps": len(unet.outs), "stepped": stepped, "generic_stepped": sch.step_index, "replay_off": replay_off,
            "finite": bool(torch.isfinite(fused).all().item()), "elem": _lib.ELEM_NAME,
            "ratio": ((fused.double() - generic).abs() / E[-1]).max().item()}



if __name__ == "__main__":
    main("MULTISTEP_JSON", [(k, (lambda k=k: run_case(k))) for k in MB.CASES] + [("graph", run_graph), ("refusals", run_refusals)],
         [("pipeline", run_pipeline)])
