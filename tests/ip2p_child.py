"""Child process of tests/test_gpu_ip2p.py (started through tests/gpu_child.py RUNNER; one element type per process).

    ip2p_child.py kernel          mi355x_sd_guidance3 and mi355x_sd_ip2p_input over the matrices of tests/ip2p_cases.py -> IP2P_JSON
    ip2p_child.py loop REFS.pt    the InstructPix2Pix loop on the miniature 8-channel U-Nets against the references the parent computed
                                  on the CPU -> IP2P_JSON

Every output buffer is a canary (7.25) with PAD floats in front of and behind the written span, which must keep their bits, as must the
inputs. "off4" cases start every operand 4 bytes behind a 16-byte boundary, which takes the element-by-element path. Every kernel
call goes through its checked wrapper (paddlemix_amd.ops.guidance3 / ip2p_input).

The loops against the restatement run on the CPU around the oracle U-Net: DPM-Solver multistep draws nothing and its reference comes
from the parent; Euler a draws one plane per step from the call's device generator, so the child draws the same planes from the same
seed, copies them to the host and hands them to the restatement through ``step``'s ``noise=``.

Nothing is caught: a failing device call raises, the child ends with a non-zero status, and no further case is launched."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlemix_amd import ops   # noqa: E402
from tests import ip2p_bounds as IB   # noqa: E402
from tests import ip2p_cases as C   # noqa: E402
from tests.bound_pieces import check, exact_off   # noqa: E402
from tests.gpu_child import emit   # noqa: E402

PAD, CANARY = 8, 7.25


def _dev(host, off):
    """host [..] fp32 -> (device buffer, view of the payload at 16 bytes * k + 4 * off)"""
    buf = torch.full((host.numel() + 2 * PAD + 4,), CANARY, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + host.numel()]
    view.copy_(host.flatten())
    return buf, view


def _untouched(buf, view_numel, off):
    b = buf.cpu()
    return int((b[:PAD + off] != CANARY).sum() + (b[PAD + off + view_numel:] != CANARY).sum())


def run_guidance3(spec, gr, form):
    batch, n, off, sigma = spec["batch"], spec["n"], spec.get("off", 0), spec.get("sigma")
    seed = 1000 * batch + n % 997
    x0 = form == "x0"
    eps = IB.cancelling_inputs(batch, n, C.GS, C.GI, seed, offset=50.0 if form == "eps" else 0.0)
    x = None
    if x0:
        x = 50.0 + torch.randn(batch, n, generator=torch.Generator().manual_seed(seed + 1))
    ref, e = IB.guidance3(eps, C.GS, C.GI, gr, x, sigma)
    ebuf, ev = _dev(eps, off)
    xbuf, xv = _dev(x, off) if x0 else (None, None)
    coef = torch.tensor([sigma if x0 else 0.0, CANARY], dtype=torch.float32, device="cuda")
    outs = []
    for _ in range(2):
        obuf, ov = _dev(torch.full((batch, n), CANARY), off)
        ops.guidance3(ev.reshape(3 * batch, n), C.GS, C.GI, gr, x=xv.reshape(batch, n) if x0 else None, sigma=coef if x0 else None,
                      out=ov.reshape(batch, n))   # the checked wrapper: a refusal raises
        torch.cuda.synchronize()
        outs.append((ov.cpu().reshape(batch, n), _untouched(obuf, batch * n, off)))
    ratio, _ = check(outs[0][0], ref, e, f32_rel=0.0)
    inputs_off = exact_off(ev.cpu().reshape(eps.shape), eps) + (exact_off(xv.cpu().reshape(x.shape), x) if x0 else 0)
    return dict(ratio=ratio, bound_finite=bool(torch.isfinite(e).all()), padding_off=outs[0][1] + outs[1][1] + _untouched(ebuf, eps.numel(), off),
                inputs_off=inputs_off, rerun_off=exact_off(outs[0][0], outs[1][0]), vector=int(ev.data_ptr() % 16 == 0 and (batch * n) % 4 == 0))


def run_input(spec):
    g, b, cl, ci, h, w, scale = (spec[k] for k in ("groups", "batch", "c_lat", "c_img", "h", "w", "scale"))
    gen = torch.Generator().manual_seed(g * 100 + b * 10 + h)
    x, img = torch.randn(b, cl, h, w, generator=gen), torch.randn(g * b, ci, h, w, generator=gen)
    want = torch.cat([scale * torch.cat([x] * g), img], dim=1)   # concat([latents] * 3), the scale, the channel concat
    _, xv = _dev(x, 0)
    _, iv = _dev(img, 0)
    obuf, ov = _dev(torch.full(tuple(want.shape), CANARY), 0)
    ops.ip2p_input(xv.reshape(x.shape), iv.reshape(img.shape), scale, out=ov.reshape(want.shape))
    torch.cuda.synchronize()
    return dict(off=exact_off(ov.cpu().reshape(want.shape), want), padding_off=_untouched(obuf, want.numel(), 0),
                inputs_off=exact_off(xv.cpu().reshape(x.shape), x) + exact_off(iv.cpu().reshape(img.shape), img))


def kernel_main():
    ops.init(0)
    out = dict(flat={}, rescale={}, input={})
    for name, spec in C.FLAT.items():
        out["flat"][name] = run_guidance3(spec, 0.0, "flat")
    for name, spec in C.RESCALE.items():
        out["rescale"][name] = run_guidance3(spec, C.GR, name.split()[0])
    for name, spec in C.INPUT.items():
        out["input"][name] = run_input(spec)
    emit("IP2P_JSON", out)


def loop_main(refs_path):
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel
    from tests import ip2p_ref as R
    from tests.step_pieces import Recording, Replay
    refs = torch.load(refs_path)
    cu = lambda v: None if v is None else ({k: t.cuda() for k, t in v.items()} if isinstance(v, dict) else v.cuda())  # noqa: E731
    rel = lambda a, r: ((a.double().cpu() - r.double().cpu()).norm() / r.double().cpu().norm()).item()  # noqa: E731
    out = {}
    for name, r in refs.items():
        cfg, sched = C.UNETS[r["unet"]], r["sched"]
        pe, ne, il, lat, added, neg = (cu(v) for v in r["inputs"])
        unet = Recording(UNet2DConditionModel(cfg, r["params"], use_graph=False))

        def call(u, **kw):
            pipe = StableDiffusionDenoiser(u, C.SCHEDULERS[sched]())
            kw = dict(dict(num_inference_steps=C.STEPS, guidance_scale=C.GS, image_guidance_scale=C.GI, latents=lat.clone(), image=il,
                           added_cond_kwargs=added, negative_added_cond_kwargs=neg,
                           generator=torch.Generator(device="cuda").manual_seed(11)), **kw)
            return pipe(pe, ne, **kw)

        def plain():   # a plain forward of the same U-Net at the text2img batch (a text2img LOOP needs in_channels == out_channels)
            return unet.unet(torch.cat([lat, il], dim=1), 501, encoder_hidden_states=pe, added_cond_kwargs=added, return_dict=False)[0].clone()
        before = plain()                           # before ...
        fused = call(unet)
        outs = list(unet.outs)
        after = plain()                            # ... and after an InstructPix2Pix call

        def replay():   # the recorded outputs in the `unet` slot; the loop reaches the library through its `unet`
            rp = Replay(unet.config, outs, dtype=torch.float32)
            rp._lib, rp._emulated = unet._lib, unet._emulated
            return rp
        unfused = call(replay(), fused_update=False)
        torch_ops = R.loop(replay(), C.SCHEDULERS[sched](), pe, ne, il, lat, C.STEPS, C.GS, C.GI, added=added, negative_added=neg,
                           generator=torch.Generator(device="cuda").manual_seed(11))
        gi1, gi25 = call(unet, image_guidance_scale=1.0), call(unet, image_guidance_scale=2.5)
        res = dict(forward_in_place_of_text2img_equal=bool(torch.equal(before, after)) and bool(torch.isfinite(before).all()), fused_vs_unfused_close=bool(torch.allclose(fused, unfused, rtol=2e-5, atol=2e-5)),
                   fused_vs_unfused=float((fused - unfused).abs().max()), fused_vs_torch_ops_close=bool(torch.allclose(fused, torch_ops, rtol=2e-5, atol=2e-5)),
                   fused_vs_torch_ops=float((fused - torch_ops).abs().max()), moved=rel(gi25, gi1))
        ref = r.get("ref")
        if ref is None:   # Euler a: the device generator's per-step draws, on the host
            from oracle import unet_ref as U
            gen = torch.Generator(device="cuda").manual_seed(11)
            noises = [torch.randn(lat.shape, generator=gen, device="cuda", dtype=torch.float32).cpu() for _ in range(C.STEPS)]
            P, host = r["params"], r["inputs"]
            oracle = lambda x, t, encoder_hidden_states, added_cond_kwargs, return_dict: (  # noqa: E731
                U.unet_forward(P, cfg, x, float(t), encoder_hidden_states, added_cond_kwargs=added_cond_kwargs),)
            ref = R.loop(oracle, C.SCHEDULERS[sched](), *host[:4], C.STEPS, C.GS, C.GI, added=host[4], negative_added=host[5], noises=noises)
        live_unfused = call(unet, fused_update=False)
        res.update(rel_fused=rel(fused, ref), rel_unfused=rel(live_unfused, ref))
        out[name] = res
    emit("IP2P_JSON", out)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel_main()
    else:
        loop_main(sys.argv[2])
