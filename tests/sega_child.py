"""Child process of tests/test_gpu_sega.py (started through tests/gpu_child.py RUNNER; one element type per process).

    sega_child.py kernel    mi355x_sd_sega_guidance over the matrix of tests/sega_cases.py -> SEGA_JSON
    sega_child.py loop      the semantic-guidance loop on the tiny U-Net, fused against fused_guidance=False -> SEGA_JSON

Every written buffer is a canary (7.25) with PAD floats in front of and behind the written span, which must keep their bits, as must
eps, extra and the row. "off4" cases start every operand 4 bytes behind a 16-byte boundary, which takes the element-by-element
selection. Every kernel call goes through its checked wrapper (paddlemix_amd.ops.sega_guidance).

Nothing is caught: a failing device call raises, the child ends with a non-zero status, and no further case is launched."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlemix_amd import ops   # noqa: E402
from tests import sega_bounds as SB   # noqa: E402
from tests import sega_cases as C   # noqa: E402
from tests.abi_emulator_sega import parse_row   # noqa: E402
from tests.bound_pieces import exact_off   # noqa: E402
from tests.gpu_child import emit   # noqa: E402

PAD, CANARY = 8, 7.25


def _dev(host, off, dtype=torch.float32):
    """host [..] -> (device buffer, view of the payload at 16 bytes * k + 4 * off)"""
    buf = torch.full((host.numel() + 2 * PAD + 4,), CANARY, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + host.numel()]
    view.view(dtype).copy_(host.flatten())
    return buf, view


def _untouched(buf, view_numel, off):
    b = buf.cpu()
    return int((b[:PAD + off] != CANARY).sum() + (b[PAD + off + view_numel:] != CANARY).sum())


def run_case(name, spec):
    n, B, Cc, hw, off = spec["n"], spec["batch"], spec["channels"], spec["hw"], spec["off"]
    eps, mom, extra, row = C.kernel_inputs(spec, seed=sorted(C.KERNEL).index(name))
    ref = SB.reference(eps, mom, extra, row.numpy(), n, spec["q"])
    ebuf, ev = _dev(eps, off)
    xbuf, xv = _dev(extra, off) if extra is not None else (None, None)
    rbuf, rv = _dev(row, off, torch.int32)
    runs = []
    for _ in range(2):
        mbuf, mv = _dev(mom, off)
        obuf, ov = _dev(torch.full((B, Cc, hw), CANARY), off)
        sbuf, sv = _dev(torch.full((n, B, Cc, 3), CANARY), off)
        ops.sega_guidance(ev.reshape((2 + n) * B, Cc, hw, 1), mv.reshape(B, Cc, hw, 1), rv, n, extra=None if xv is None else xv.reshape(B, Cc, hw, 1),
                          out=ov.reshape(B, Cc, hw, 1), stats=sv.reshape(n, B, Cc, 3))   # the checked wrapper: a refusal raises
        torch.cuda.synchronize()
        runs.append(dict(out=ov.cpu().reshape(B, Cc, hw), mom=mv.cpu().reshape(B, Cc, hw), stats=sv.cpu().reshape(n, B, Cc, 3),
                         pad=_untouched(obuf, B * Cc * hw, off) + _untouched(mbuf, B * Cc * hw, off) + _untouched(sbuf, 3 * n * B * Cc, off)))
    a, b = runs
    live = [c for c in range(n) if (parse_row(row.numpy(), n)["active"] >> c) & 1]
    dead = [c for c in range(n) if c not in live]
    st = a["stats"]
    bits = lambda t: torch.nan_to_num(t, nan=-1.0).contiguous().view(torch.int32)   # noqa: E731
    order_off = exact_off(bits(st[live][..., 0]), bits(ref["vlo"][live])) + exact_off(bits(st[live][..., 1]), bits(ref["vhi"][live]))
    thr_off = SB.check_thr(st[live][..., 2], ref["vlo"][live], ref["vhi"][live], ref["thr64"][live]) if live else 0
    # the mask the kernel applied: |g| (the reference's two roundings, the kernel's keys bit for bit) against the kernel's own threshold
    mask_off = 0
    for c in live:
        g = ((eps[2 + c] - eps[0]) * torch.tensor(float(parse_row(row.numpy(), n)["per"][c]["scale"]))).abs()
        mask_off += int(((g >= st[c, ..., 2][..., None]) != ref["mask"][c]).sum())
    r_out, cls_out = SB.check_values(a["out"], ref["out"], ref["e_out"])
    r_mom, cls_mom = SB.check_values(a["mom"], ref["mom"], ref["e_mom"])
    inputs_off = exact_off(ev.cpu().reshape(eps.shape), eps) + exact_off(rv.cpu().view(torch.int32), row) + \
        (exact_off(xv.cpu().reshape(extra.shape), extra) if extra is not None else 0)
    return dict(order_off=order_off, thr_off=thr_off, mask_off=mask_off, near=ref["near"], ratio_out=r_out, ratio_mom=r_mom,
                class_off=cls_out + cls_mom, dead_stats_off=int((st[dead] != 0).sum()) if dead else 0,
                padding_off=a["pad"] + b["pad"] + _untouched(ebuf, eps.numel(), off) + _untouched(rbuf, row.numel(), off),
                inputs_off=inputs_off,
                rerun_off=exact_off(bits(a["out"]), bits(b["out"])) + exact_off(bits(a["mom"]), bits(b["mom"])) + exact_off(bits(a["stats"]), bits(b["stats"])),
                vector=int(ev.data_ptr() % 16 == 0 and hw % 4 == 0))


def kernel_main():
    ops.init(0)
    emit("SEGA_JSON", {name: run_case(name, spec) for name, spec in C.KERNEL.items()})


def loop_main():
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests import configs
    from tests.step_pieces import Recording, Replay
    cfg = configs.TINY
    P = {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in synth_unet_params(cfg, seed=1234).items()}
    g = torch.Generator().manual_seed(3)
    B, hw, T, D = 2, 16, 7, cfg["cross_attention_dim"]
    pe, ne = torch.randn(B, T, D, generator=g).cuda(), torch.randn(B, T, D, generator=g).cuda()
    ee = (torch.randn(2, B, T, D, generator=g) + torch.tensor([0.5, -0.5])[:, None, None, None]).cuda()
    lat, sem = torch.randn(B, 4, hw, hw, generator=g).cuda(), (0.05 * torch.randn(4, B, 4, hw, hw, generator=g)).cuda()
    edit = dict(reverse_editing_direction=[False, True], edit_guidance_scale=[5.0, 4.0], edit_warmup_steps=[0, 2], edit_cooldown_steps=[3, 5],
                edit_threshold=[0.9, 0.75], edit_weights=[1.0, 0.5], edit_momentum_scale=0.3, edit_mom_beta=0.4)
    out = {}
    for sched in ("ddim", "dpm"):
        unet = Recording(UNet2DConditionModel(cfg, P, use_graph=False))

        def call(u, **kw):
            pipe = StableDiffusionDenoiser(u, C.SCHEDULERS[sched]())
            return pipe(pe, ne, num_inference_steps=4, guidance_scale=C.GS, latents=lat.clone(), editing_prompt_embeds=ee,
                        **{**edit, "sem_guidance": sem, **kw})
        fused = call(unet)
        rp = Replay(unet.config, list(unet.outs), dtype=torch.float32)   # the same U-Net outputs under the torch-op guidance
        rp._lib, rp._emulated = unet._lib, unet._emulated
        torch_ops = call(rp, fused_guidance=False)
        plain = call(unet, edit_guidance_scale=[0.0, 0.0], sem_guidance=None)
        scale = float(fused.abs().max())
        out[sched] = dict(diff=float((fused - torch_ops).abs().max()), scale=scale, finite=bool(torch.isfinite(fused).all()),
                          moved=float((fused - plain).abs().max()))
    emit("SEGA_JSON", out)


if __name__ == "__main__":
    kernel_main() if sys.argv[1] == "kernel" else loop_main()
