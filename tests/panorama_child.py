"""Child process of tests/test_gpu_panorama.py (started through tests/gpu_child.py RUNNER; one element type per process).

    panorama_child.py kernel          mi355x_sd_view_input / mi355x_sd_view_merge over the matrix of tests/panorama_cases.py -> PANO_JSON
    panorama_child.py loop REFS.pt    the panorama loop on the tiny U-Net -> PANO_JSON

Every written buffer is a canary (7.25) with PAD floats in front of and behind the written span, which must keep their bits, as must
the inputs. "off4" cases start every operand 4 bytes behind a 16-byte boundary, which takes the element-by-element path. Every kernel
call goes through its checked wrapper (paddlemix_amd.ops.view_input / view_merge).

Nothing is caught: a failing device call raises, the child ends with a non-zero status, and no further case is launched."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlemix_amd import ops   # noqa: E402
from tests import panorama_cases as C   # noqa: E402
from tests import panorama_ref as R   # noqa: E402
from tests.gpu_child import emit   # noqa: E402

PAD, CANARY = 8, 7.25


def _dev(host, off):
    """host [..] -> (device buffer, view of the payload at 16 bytes * k + 4 * off)"""
    buf = torch.full((host.numel() + 2 * PAD + 4,), CANARY, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + host.numel()]
    view.copy_(host.flatten())
    return buf, view


def _untouched(buf, view_numel, off):
    b = buf.cpu()
    return int((b[:PAD + off] != CANARY).sum() + (b[PAD + off + view_numel:] != CANARY).sum())


def bits_off(a, b):
    """elements whose bits differ, a NaN matching a NaN; every element is compared"""
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(((a.view(torch.int32) != b.view(torch.int32)) & ~(torch.isnan(a) & torch.isnan(b))).sum())


def run_case(name, spec):
    B, Cc, H, W, off = spec["batch"], spec["C"], spec["H"], spec["W"], spec["off"]
    window, counts, stride, circular = (spec["win_h"], spec["win_w"]), (spec["ny"], spec["nx"]), spec["stride"], bool(spec["circular"])
    x, views = C.kernel_inputs(spec, seed=sorted(C.KERNEL).index(name))
    xbuf, xv = _dev(x, off)
    vbuf, vv = _dev(views, off)
    res = dict(input_off=0, merge_off=0, padding_off=0, rerun_off=0)
    for groups in (1, 2):
        ref = R.kernel_reference(spec, x, views, C.SCALE, groups)
        runs = []
        for _ in range(2):
            obuf, ov = _dev(torch.full(ref["input"].shape, CANARY), off)
            ops.view_input(xv.reshape(x.shape), window, stride, counts, scale=C.SCALE, groups=groups, circular=circular,
                           first=ref["first"], count=ref["n"], out=ov.reshape(ref["input"].shape))   # the checked wrapper: a refusal raises
            torch.cuda.synchronize()
            runs.append(ov.cpu().reshape(ref["input"].shape))
            res["padding_off"] += _untouched(obuf, ref["input"].numel(), off)
        res["input_off"] += bits_off(runs[0], ref["input"])
        res["rerun_off"] += bits_off(runs[0], runs[1])
    runs = []
    for _ in range(2):
        obuf, ov = _dev(torch.full(x.shape, CANARY), off)
        ops.view_merge(vv.reshape(views.shape), x.shape, stride, counts, circular=circular, out=ov.reshape(x.shape))
        torch.cuda.synchronize()
        runs.append(ov.cpu().reshape(x.shape))
        res["padding_off"] += _untouched(obuf, x.numel(), off)
    res["merge_off"] = bits_off(runs[0], ref["merged"])
    res["rerun_off"] += bits_off(runs[0], runs[1])
    res["padding_off"] += _untouched(xbuf, x.numel(), off) + _untouched(vbuf, views.numel(), off)
    res["inputs_off"] = bits_off(xv.cpu().reshape(x.shape), x) + bits_off(vv.cpu().reshape(views.shape), views)
    res["negzero_plus"] = bool(runs[0][0, 0, 0, 1].view(torch.int32).item() == 0 and ref["count"][0, 0, 0, 1] > 0)
    res["uncovered"] = int((ref["count"] == 0).sum())
    res["uncovered_plus_zero"] = bool((runs[0][ref["count"] == 0].view(torch.int32) == 0).all())
    res["max_count"], res["recip"], res["odd_counts"] = int(ref["count"].max()), ref["recip"], ref["odd_counts"]
    res["vector"] = int(xv.data_ptr() % 16 == 0 and vv.data_ptr() % 16 == 0 and W % 4 == 0 and spec["win_w"] % 4 == 0 and stride % 4 == 0)
    return res


def kernel_main():
    ops.init(0)
    emit("PANO_JSON", {name: run_case(name, spec) for name, spec in C.KERNEL.items()})


class Recorder:
    """a U-Net wrapper that keeps every input and output of a run"""

    def __init__(self, unet):
        self.unet, self.config, self._lib, self._emulated, self.ins, self.outs = unet, unet.config, unet._lib, unet._emulated, [], []

    def __call__(self, x, *args, **kwargs):
        out = self.unet(x, *args, **kwargs)
        self.ins.append(x.detach().clone())
        self.outs.append(out[0].detach().clone())
        return out


class CheckedReplay:
    """in the `unet` slot: returns the recorded outputs in order (plus `bump` on sample `bump_at` of the first call) and counts the
    inputs whose bits are not the recorded ones"""

    def __init__(self, rec, bump=0.0, bump_at=0):
        self.config, self._lib, self._emulated, self.rec, self.i, self.input_off = rec.config, rec._lib, rec._emulated, rec, 0, 0
        self.bump, self.bump_at = bump, bump_at

    def __call__(self, x, *args, **kwargs):
        self.input_off += bits_off(x, self.rec.ins[self.i])
        out = self.rec.outs[self.i].clone()
        if self.i == 0 and self.bump:
            out[self.bump_at] += self.bump
        self.i += 1
        return (out,)


def loop_main(refs_path):
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel
    from tests import configs
    refs = torch.load(refs_path)
    cfg = configs.TINY
    rel = lambda a, r: ((a.double().cpu() - r.double().cpu()).norm() / r.double().cpu().norm()).item()  # noqa: E731
    out = {}
    for name, r in refs.items():
        pe, ne, lat = (v.cuda() for v in r["inputs"])
        rec = Recorder(UNet2DConditionModel(cfg, r["params"], use_graph=False))

        def call(u, **kw):
            pipe = StableDiffusionDenoiser(u, C.SCHEDULERS[r["sched"]]())
            return pipe(pe, ne, num_inference_steps=C.STEPS, guidance_scale=C.GS, latents=lat.clone(), panorama=True,
                        circular_padding=r["circular"], **kw)
        fused = call(rec)
        rp = CheckedReplay(rec)
        torch_ops = call(rp, fused_views=False)
        # (c) the text group's output of view 1 moved on the first step: the result moves inside that view's window and nowhere else
        views_n = len(rec.ins[0]) // 2
        moved = call(CheckedReplay(rec, bump=0.5, bump_at=views_n + 1))
        d = (moved - fused).abs()[0].amax(dim=(0, 1)).cpu()            # per column
        inside = torch.zeros(lat.shape[3], dtype=torch.bool)
        inside[(torch.arange(64) + 8) % lat.shape[3]] = True           # view 1: columns 8 .. 71
        out[name] = dict(views_off=bits_off(fused, torch_ops), unet_input_off=rp.input_off, rel=rel(fused, r["ref"]),
                         finite=bool(torch.isfinite(fused).all()), moved_inside=float(d[inside].min()), moved_outside=float(d[~inside].max()),
                         unet_calls=len(rec.outs))
    emit("PANO_JSON", out)


if __name__ == "__main__":
    kernel_main() if sys.argv[1] == "kernel" else loop_main(sys.argv[2])
