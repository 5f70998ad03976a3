"""Child process of tests/test_gpu_adapter.py (started through tests/gpu_child.py RUNNER; one element type per process).

    adapter_child.py kernel           mi355x_sd_pixel_unshuffle / _avgpool2 / _relu over their case lists on the build MI355X_SD_DTYPE
                                      selects -> ADAPTER_JSON
    adapter_child.py model REFS.pt    the three adapter types, the U-Net with intrablock residuals and one pipeline call against the
                                      references the parent computed on the CPU -> ADAPTER_JSON

Every buffer is a canary outside what the entry writes (row padding, two rows behind the end); those must keep their bits.
Nothing is caught: a failing device call raises, the child ends with a non-zero status, and no further case is launched."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import bound_pieces as BP   # noqa: E402
from tests.gpu_child import emit, sha   # noqa: E402

CANARY = 7.25
# (B, C, H, W, r, columns of padding behind C r^2): the issue's three, one of them again with padded rows, and an r that is no
# multiple of 8 (the element-by-element form)
UNSHUFFLE = {"2x3x16x24-r8": (2, 3, 16, 24, 8, 0), "1x1x32x16-r16": (1, 1, 32, 16, 16, 0), "2x3x32x32-r16": (2, 3, 32, 32, 16, 0),
             "2x3x16x24-r8-pad": (2, 3, 16, 24, 8, 16), "2x2x6x10-r2": (2, 2, 6, 10, 2, 8)}
# (B, H, W, C, columns of padding behind C in x and y): even, odd both, a single pixel, odd x even; padded rows; more than one block
AVGPOOL = {"2x6x10x64": (2, 6, 10, 64, 0), "2x5x7x64": (2, 5, 7, 64, 0), "1x1x1x8": (1, 1, 1, 8, 0), "1x9x2x72": (1, 9, 2, 72, 0),
           "2x5x7x64-pad": (2, 5, 7, 64, 8), "2x33x17x72-pad": (2, 33, 17, 72, 8)}
# (rows, C, padding, in place): vector and element forms, in place and out of place
RELU = {"37x64": (37, 64, 0, False), "37x64-inplace": (37, 64, 0, True), "37x64-pad-inplace": (37, 64, 8, True), "5x13": (5, 13, 3, False),
        "5x13-inplace": (5, 13, 3, True), "1200x72": (1200, 72, 8, False)}


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _untouched(out, host, keep):
    return int((_bits(out)[keep] != _bits(host)[keep]).sum())


def unshuffle_case(lib, dt, B, C, H, W, r, pad):
    from paddlemix_amd import _lib
    K, rows = C * r * r, B * (H // r) * (W // r)
    ld = K + pad
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    host = torch.full((rows + 2, ld), CANARY, dtype=dt)
    dev, xd = host.cuda(), x.cuda()
    _lib.check(lib.mi355x_sd_pixel_unshuffle(xd.data_ptr(), B, C, H, W, r, dev.data_ptr(), ld, 0))
    torch.cuda.synchronize()
    out = dev.cpu()
    want = torch.pixel_unshuffle(x, r).permute(0, 2, 3, 1).reshape(rows, K).to(dt)
    keep = torch.ones(rows + 2, ld, dtype=torch.bool)
    keep[:rows, :K] = False
    return dict(off=BP.exact_off(out[:rows, :K].contiguous(), want), untouched_off=_untouched(out, host, keep))


def avgpool_case(lib, dt, B, H, W, C, pad):
    """float64 reference of the stored inputs; e = 3 * 2^-24 * the mean of |x| over the window: an fp32 sum of at most 4 terms (3
    additions, each within 2^-24 of the running sum of magnitudes) and an exact scale"""
    from paddlemix_amd import _lib
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ldx = ldy = C + pad
    g = torch.Generator().manual_seed(H * 100 + W)
    xin = torch.full((B * H * W + 2, ldx), CANARY, dtype=dt)
    xin[:B * H * W, :C] = (torch.randn(B * H * W, C, generator=g) * torch.logspace(-3, 3, C)[None, :]).to(dt)
    host = torch.full((B * Ho * Wo + 2, ldy), CANARY, dtype=dt)
    dev, xd = host.cuda(), xin.cuda()
    _lib.check(lib.mi355x_sd_avgpool2(xd.data_ptr(), ldx, B, H, W, C, dev.data_ptr(), ldy, 0))
    torch.cuda.synchronize()
    out = dev.cpu()
    x64 = xin[:B * H * W, :C].double().reshape(B, H, W, C).permute(0, 3, 1, 2)
    pool = lambda t: torch.nn.functional.avg_pool2d(t, 2, 2, ceil_mode=True, count_include_pad=False)  # noqa: E731
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)  # noqa: E731
    ref, e = back(pool(x64)), back(3 * BP.U32 * pool(x64.abs()))
    ratio, rel = BP.check(out[:B * Ho * Wo, :C], ref, e)
    keep = torch.ones(B * Ho * Wo + 2, ldy, dtype=torch.bool)
    keep[:B * Ho * Wo, :C] = False
    return dict(ratio=ratio, rel=rel, untouched_off=_untouched(out, host, keep), shape=[Ho, Wo])


def relu_case(lib, dt, rows, C, pad, inplace):
    from paddlemix_amd import _lib
    ld = C + pad
    g = torch.Generator().manual_seed(rows + C)
    x = torch.full((rows + 2, ld), CANARY, dtype=dt)
    v = torch.randn(rows, C, generator=g) * torch.logspace(-30, 30, C)[None, :]      # tiny and large magnitudes, both signs
    v[0, :4] = torch.tensor([0.0, -0.0, torch.finfo(dt).max, -torch.finfo(dt).max])
    v[1, :2] = torch.tensor([torch.finfo(dt).tiny, -torch.finfo(dt).tiny])
    x[:rows, :C] = v.clamp(-torch.finfo(dt).max, torch.finfo(dt).max).to(dt)
    xd = x.cuda()
    yd = xd if inplace else torch.full((rows + 2, ld), CANARY, dtype=dt).cuda()
    _lib.check(lib.mi355x_sd_relu(xd.data_ptr(), ld, yd.data_ptr(), ld, rows, C, 0))
    torch.cuda.synchronize()
    out = yd.cpu()
    want = torch.relu(x[:rows, :C].float())
    assert torch.isfinite(want).all()
    keep = torch.ones(rows + 2, ld, dtype=torch.bool)
    keep[:rows, :C] = False
    base = x if inplace else torch.full((rows + 2, ld), CANARY, dtype=dt)
    return dict(unequal=int((out[:rows, :C].float() != want).sum()), untouched_off=_untouched(out, base, keep),
                input_off=0 if inplace else _untouched(xd.cpu(), x, torch.ones(rows + 2, ld, dtype=torch.bool)))


def kernel_main():
    from paddlemix_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mi355x_sd_init(0))
    dt = _lib.elem_dtype()
    out = {"unshuffle": {k: unshuffle_case(lib, dt, *v) for k, v in UNSHUFFLE.items()}}
    out["avgpool"] = {k: avgpool_case(lib, dt, *v) for k, v in AVGPOOL.items()}
    out["relu"] = {k: relu_case(lib, dt, *v) for k, v in RELU.items()}
    emit("ADAPTER_JSON", out)


def model_main(refs_path):
    from paddlemix_amd.adapter import T2IAdapter
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import DDIMScheduler
    from paddlemix_amd.unet import UNet2DConditionModel
    refs = torch.load(refs_path)
    rel = lambda a, r: ((a.double().cpu() - r.double()).norm() / r.double().norm()).item()  # noqa: E731
    cu = lambda x: None if x is None else ({k: v.cuda() for k, v in x.items()} if isinstance(x, dict) else x.cuda())  # noqa: E731
    out = {"adapter": {}, "unet": {}}
    for name, r in refs["adapter"].items():
        net = T2IAdapter(r["config"], r["params"])
        feats = net(r["image"].cuda())
        again = net(r["image"].cuda())
        out["adapter"][name] = dict(rel=[rel(f, g) for f, g in zip(feats, r["ref"])], shapes=[list(f.shape) for f in feats],
                                    n_ref=len(r["ref"]), fp32=all(f.dtype == torch.float32 for f in feats),
                                    rerun_equal=all(torch.equal(a, b) for a, b in zip(feats, again)))
    adapters = {}
    for name, r in refs["unet"].items():
        res = {}
        for graph in (False, True):
            m = UNet2DConditionModel(r["cfg"], r["params"], use_graph=graph)
            call = lambda **kw: m(cu(r["sample"]), 501, cu(r["enc"]), added_cond_kwargs=cu(r["added"]), **kw).sample.cpu()  # noqa: E731
            plain = call()
            rs = [t.cuda() for t in r["residuals"]]
            on = call(down_intrablock_additional_residuals=list(rs))
            dep = call(down_block_additional_residuals=list(rs))
            zero = call(down_intrablock_additional_residuals=[torch.zeros_like(t) for t in rs])
            res["graph" if graph else "eager"] = dict(
                rel_on=rel(on, r["ref_on"]), rel_plain=rel(plain, r["ref_plain"]), on_vs_plain=rel(on, plain),
                zero_equals_plain=bool(torch.equal(zero, plain)), deprecated_equals_intrablock=bool(torch.equal(dep, on)),
                plain_after_equals_plain=bool(torch.equal(call(), plain)), plans=len(m._plans), sha_on=sha(on))
        res["graph_equals_eager"] = res["graph"]["sha_on"] == res["eager"]["sha_on"]
        # (iv) an odd latent with the adapter's own features: every pool is a ceil-mode one and the shapes must meet the U-Net's
        o = r["odd"]
        ad = adapters[name] = T2IAdapter(o["adapter_config"], o["adapter_params"])
        feats = ad(o["image"].cuda())
        m = UNet2DConditionModel(r["cfg"], r["params"])
        got = m(cu(o["sample"]), 501, cu(o["enc"]), added_cond_kwargs=cu(o["added"]), down_intrablock_additional_residuals=feats).sample
        res["odd"] = dict(rel=rel(got, o["ref"]), feature_shapes=[list(f.shape) for f in feats], adds=len(list(m._plans.values())[-1].intra))
        out["unet"][name] = res
    if "pipeline" not in refs:   # (the fp16 build: the adapters only)
        return emit("ADAPTER_JSON", out)
    # pipeline: 4 steps with the adapter and CFG on the SD-1.5 shape
    p = refs["pipeline"]
    r = refs["unet"]["sd15"]
    sched = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionDenoiser(UNet2DConditionModel(r["cfg"], r["params"]), DDIMScheduler(**sched), adapter=adapters["sd15"])
    run = lambda **kw: pipe(p["pe"].cuda(), p["ne"].cuda(), num_inference_steps=4, guidance_scale=5.0, latents=p["lat0"].cuda(), **kw).cpu()  # noqa: E731
    plain = run()
    on = run(adapter_image=p["image"].cuda())
    off = run(adapter_image=p["image"].cuda(), adapter_conditioning_factor=0.0)
    out["pipeline"] = dict(finite=bool(torch.isfinite(on).all()), on_vs_plain=rel(on, plain), factor0_equals_plain=bool(torch.equal(off, plain)))
    emit("ADAPTER_JSON", out)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel_main()
    else:
        model_main(sys.argv[2])
