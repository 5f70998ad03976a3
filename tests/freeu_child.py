"""Child process of tests/test_gpu_freeu.py (started through tests/gpu_child.py RUNNER; one element type per process).

    freeu_child.py kernel          mi355x_sd_freeu over the CASES matrix on the build MI355X_SD_DTYPE selects -> FREEU_JSON
    freeu_child.py unet REFS.pt    whole U-Nets with FreeU against the references the parent computed on the CPU, the C handle and an
                                   exported program against the Python-planned model -> FREEU_JSON

The kernel cases: every plane size of the issue plus the smallest one the row split engages on (freeu_bounds.SPLIT_SHAPE), B = 2,
ld > Cx + Cs, three channel layouts -- aligned, an odd Cx (every skip group of the first and last 16 bytes straddles a boundary),
Cx = 0 with a Cs that is no vector multiple --, 16-bit and fp32 elements, six input kinds. Those layouts are at most 64 column groups
wide, one grid column; the "wide" layout (freeu_bounds.WIDE_CHANNELS, at 2 x 2 and 3 x 5) makes both the backbone half and the skip
span several grid columns with a ragged last one, as every production shape is. The buffer is a canary outside the written columns;
the padding, the untouched backbone half and two rows behind the end must keep their bits.

The pure cos (ty - tx) plane "must come back as its input rounded once". With fp32 elements the plane is pure to 2^-24 and the
reference IS the input, held to the same bound. A plane rounded to 16 bits is no longer pure: its rounding error has components in
every bin, which the filter does scale, so there the reference is the float64 filter of the rounded plane the kernel was given,
like every other input kind -- not the input itself.

Nothing is caught: a failing device call raises, the child ends with a non-zero status, and no further case is launched."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import freeu_bounds as FB   # noqa: E402
from tests.gpu_child import emit, sha   # noqa: E402

SHAPES = [(2, 2), (3, 5), (8, 8), (16, 12), FB.SPLIT_SHAPE]
CHANNELS = {"aligned": (16, 64), "odd-cx": (5, 64), "cx0-tail": (0, 37), "wide": FB.WIDE_CHANNELS}
CASES = {f"{H}x{W}-{cn}-{'f32' if f32 else 'e16'}": (H, W, cn, f32)
         for cn in CHANNELS for H, W in (FB.WIDE_SHAPES if cn == "wide" else SHAPES) for f32 in (0, 1)}
B = 2
CANARY = 7.25


def run_case(lib, H, W, cn, f32):
    from paddlemix_amd import _lib
    Cx, Cs = CHANNELS[cn]
    dt = torch.float32 if f32 else _lib.elem_dtype()
    vec = 4 if f32 else 8
    ld = ((Cx + Cs) // vec + 2) * vec
    rows = B * H * W
    s, b = (0.9, 1.3) if (H, W) == FB.SPLIT_SHAPE else (0.2, 1.4)
    ws = torch.empty(max(1, lib.mi355x_sd_freeu_workspace_floats(B, H, W, Cs)), dtype=torch.float32, device="cuda")
    res = dict(ratio={}, splits=FB.launch(B, H, W, Cx, Cs, bool(f32))["splits"], untouched_off=0, rerun_off=0, rc=0)
    for kind in FB.KINDS:
        host = torch.full((rows + 2, ld), CANARY, dtype=dt)
        g = torch.Generator().manual_seed(100 * H + W)
        host[:rows, :Cx] = torch.randn(rows, Cx, generator=g).to(dt)
        planes = FB.planes_input(kind, B, H, W, Cs, seed=3)
        host[:rows, Cx:Cx + Cs] = planes.permute(0, 2, 3, 1).reshape(rows, Cs).to(dt)
        ref, e = FB.expected(host[:rows], B, H, W, Cx, Cs, b, s, bool(f32))
        if kind == "cos_diff" and f32 and H > 2 and W > 2:
            ref[:, Cx:] = host[:rows, Cx:Cx + Cs].double()   # the untouched component: the input itself, rounded once by the store
        outs = []
        for _ in range(2):
            dev = host.cuda()
            ws.fill_(float("nan"))
            _lib.check(lib.mi355x_sd_freeu(dev.data_ptr(), ld, B, H, W, Cx, Cs, b, s, f32, ws.data_ptr(), 0))   # a refusal raises
            torch.cuda.synchronize()
            outs.append(dev.cpu())
        out = outs[0]
        res["rerun_off"] += int((outs[0].view(torch.int32 if f32 else torch.int16) != outs[1].view(torch.int32 if f32 else torch.int16)).sum())
        res["ratio"][kind] = FB.check(out[:rows, :Cx + Cs], ref, e)
        keep = torch.ones(rows + 2, ld, dtype=torch.bool)
        keep[:rows, :Cx // 2] = False
        keep[:rows, Cx:Cx + Cs] = False
        bits = lambda t: t.view(torch.int32 if f32 else torch.int16)  # noqa: E731
        res["untouched_off"] += int((bits(out)[keep] != bits(host)[keep]).sum())
    return res


def kernel_main():
    from paddlemix_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mi355x_sd_init(0))
    out = {}
    for name, (H, W, cn, f32) in CASES.items():   # an exception -- a device fault reaches Python as one -- ends the child: nothing more
        out[name] = run_case(lib, H, W, cn, f32)   # is launched after it, and every test of the build fails on the child's status
    emit("FREEU_JSON", out)


def unet_main(refs_path):
    import tempfile

    from paddlemix_amd.cexec import CUNet2DConditionModel
    from paddlemix_amd.export import ExportedProgram, _named_tensors, export_program
    from paddlemix_amd.unet import UNet2DConditionModel
    from tests import configs
    refs = torch.load(refs_path)
    fu = FB.FREEU
    rel = lambda a, r: ((a.double() - r.double()).norm() / r.double().norm()).item()  # noqa: E731
    cu = lambda x: None if x is None else ({k: v.cuda() for k, v in x.items()} if isinstance(x, dict) else x.cuda())  # noqa: E731
    out = {}
    for name, r in refs.items():
        cfg, P = getattr(configs, r["cfg"]), r["params"]
        sample, enc, added = r["sample"], r["enc"], r["added"]
        call = lambda m: m(cu(sample), 501, cu(enc), added_cond_kwargs=cu(added)).sample.cpu()  # noqa: E731
        res = {}
        for graph in (False, True):
            m = UNet2DConditionModel(cfg, P, use_graph=graph)
            never = call(m)
            m.enable_freeu(**fu)
            on = call(m)
            m.enable_freeu(1.0, 1.0, 1.0, 1.0)
            ones = call(m)
            m.disable_freeu()
            off = call(m)
            g = "graph" if graph else "eager"
            res[g] = dict(rel_on=rel(on, r["ref_on"]), rel_off=rel(never, r["ref_off"]), rel_on_vs_off_ref=rel(on, r["ref_off"]),
                          ones_equal_off=bool(torch.equal(ones, never)), off_after_on_equal=bool(torch.equal(off, never)),
                          plans=len(m._plans), sha_on=sha(on))
        res["graph_equals_eager"] = res["graph"]["sha_on"] == res["eager"]["sha_on"]
        if name == "tiny":
            c = CUNet2DConditionModel(cfg, P, use_graph=False)
            base = c(cu(sample), 501, cu(enc), added_cond_kwargs=cu(added)).sample.cpu()
            c.enable_freeu(**fu)
            got = c(cu(sample), 501, cu(enc), added_cond_kwargs=cu(added)).sample.cpu()
            c.disable_freeu()
            back = c(cu(sample), 501, cu(enc), added_cond_kwargs=cu(added)).sample.cpu()
            res["cexec"] = dict(on_equal=sha(got) == res["eager"]["sha_on"], off_equal=bool(torch.equal(base, never)),
                                off_after_on_equal=bool(torch.equal(back, base)))
            # an exported FreeU program replays like the live model
            m = UNet2DConditionModel(cfg, P, use_graph=False)
            m.enable_freeu(**fu)
            live = call(m)
            plan = list(m._plans.values())[-1]
            names = [getattr(fn, "__name__", "") for fn, *_ in plan.prog]
            inputs = {n: t.clone() for n, t in _named_tensors(plan) if n != "out"}
            with tempfile.TemporaryDirectory() as td:
                path = os.path.join(td, "tiny_freeu.mi3prg")
                export_program(m, plan, path, ("out",))
                prog = ExportedProgram(path).bind()
                replay = prog.run(**inputs)["out"].cpu()
                prog.close()
            res["export"] = dict(freeu_launches=names.count("mi355x_sd_freeu"), replay_equal=bool(torch.equal(replay, live)),
                                 live_is_on=sha(live) == res["eager"]["sha_on"])
        out[name] = res
    emit("FREEU_JSON", out)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel_main()
    else:
        unet_main(sys.argv[2])
