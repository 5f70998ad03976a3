"""CPU tests of FreeU (ABI 22): the closed form against the float64 FFT restatement of the reference's fourier_filter / apply_freeu
(tests/freeu_bounds.py; paddle_utils.py:259-313), the bound against three wrong closed forms, the C surface and its refusals, and
the host logic -- planner placement, plan keys, ControlNet, pipeline -- on the emulator (tests/abi_emulator_freeu.py) against the
oracle with FreeU patched into its up resnets."""
import ctypes
import json
import math
import os

import pytest
import torch

from oracle import unet_ref as U
from paddlemix_amd import _lib
from paddlemix_amd.unet import ControlNetModel, UNet2DConditionModel, _structure, normalize_config, synth_controlnet_params, synth_unet_params
from tests import freeu_bounds as FB
from tests.abi_emulator import on_emulator
from tests.abi_emulator_freeu import FreeUEmulator
from tests.configs import MINI_XL, TINY
from tests.test_host_logic import _inputs, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FU = FB.FREEU
TOL = 2e-2   # tests/test_host_logic.py test_program_matches_oracle, tests/test_gpu_unet.py test_small_unet_vs_oracle: same configs
GEOM = {"tiny": (TINY, 2, 16, 16, 7), "mini-xl": (MINI_XL, 2, 16, 16, 77)}


# ---- the form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FB.SIZES)
def test_closed_form_equals_the_fft_restatement(H, W):
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(H * 100 + W))
    for s in (0.2, 0.9, 1.7):
        assert (FB.closed_form(x, s) - FB.fourier_filter(x, 1, s)).abs().max().item() <= 1e-14
    # the two properties of the asymmetric box: ty - tx untouched; a +-1 component scaled by half of (s - 1), all of it on an axis of 2
    ty, tx = FB.angles(H, W)
    if H > 2 and W > 2:
        d = (ty - tx).cos()
        assert (FB.fourier_filter(d, 1, 0.2) - d).abs().max().item() <= 1e-14
    c = ty.cos()
    want = c * (1 + (0.2 - 1) * (1.0 if H == 2 else 0.5))
    assert (FB.fourier_filter(c, 1, 0.2) - want).abs().max().item() <= 1e-14


@pytest.mark.parametrize("mutant", ["drop_sum", "scale_diff", "full_pm1"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_the_bound_separates_wrong_forms(mutant, dt):
    """on the inputs of the GPU matrix (tests/freeu_child.py): the closed form, rounded once, is inside the bound on every one of
    them; each mutant is outside it on at least one (by a factor printed here)"""
    from tests.freeu_child import B, SHAPES
    Cx, Cs, b, s = 0, 8, 1.4, 0.2
    worst_good, worst_bad = 0.0, 0.0
    for H, W in SHAPES:
        for kind in FB.KINDS:
            rows = FB.planes_input(kind, B, H, W, Cs, seed=3).permute(0, 2, 3, 1).reshape(B * H * W, Cs).to(dt)
            ref, e = FB.expected(rows, B, H, W, Cx, Cs, b, s, dt == torch.float32)
            planes = rows.double().reshape(B, H, W, Cs).permute(0, 3, 1, 2)
            back = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, Cs).to(dt)  # noqa: E731
            worst_good = max(worst_good, FB.check(back(FB.closed_form(planes, FB.fp32(s))), ref, e))
            worst_bad = max(worst_bad, FB.check(back(FB.closed_form(planes, FB.fp32(s), mutant)), ref, e))
    print(f"{mutant} {dt}: closed form {worst_good:.3f} of the bound, mutant {worst_bad:.1f}")
    assert worst_good < 1.0 and worst_bad > 1.0


def test_launch_heuristics_engage_the_split_on_the_named_shape():
    for f32 in (False, True):
        assert FB.launch(2, *FB.SPLIT_SHAPE, 16, 64, f32)["splits"] > 1
        assert all(FB.launch(2, H, W, 16, 64, f32)["splits"] == 1 for H, W in [(2, 2), (3, 5), (8, 8), (16, 12)])
    assert FB.launch(8, 32, 32, 1280, 1280, False)["splits"] == 8   # an SDXL level: 3 grid columns x 8 batch items -> 8 row splits
    # the narrow layouts of the GPU matrix are one grid column; the wide one is several per span, the last one ragged, like SDXL's
    from tests.freeu_child import CHANNELS
    for vec in (8, 4):
        for cn, (Cx, Cs) in CHANNELS.items():
            for c0, c1 in ((0, Cx // 2), (Cx, Cx + Cs)):
                _, ng, nc, gw, _ = FB.cols(c0, c1, vec)
                assert (nc > 1 and nc * gw > ng) if cn == "wide" else nc <= 1, (cn, vec, ng, nc, gw)
    assert FB.cols(1280, 2560, 8)[1:4] == (160, 3, 54)


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_abi():
    hdr = open(os.path.join(ROOT, "include", "mi355x_sd.h")).read()
    for sym in ("mi355x_sd_freeu_workspace_floats", "mi355x_sd_freeu", "mi355x_sd_unet_set_freeu"):
        assert f" {sym}(" in hdr and sym in _lib.SIGNATURES
    abi = int(hdr.split("#define MI355X_SD_ABI_VERSION")[1].split()[0])
    assert abi == _lib.ABI_VERSION >= 22
    assert _lib.SIGNATURES["mi355x_sd_freeu"][1][1] is ctypes.c_int64 and _lib.SIGNATURES["mi355x_sd_freeu_workspace_floats"][0] is ctypes.c_int64
    lib = _lib.load()
    assert lib.mi355x_sd_abi_version() == abi
    for args in [(2, 16, 12, 64), (8, 64, 64, 1280), (1, 2, 2, 1), (2, 40, 4, 37)]:
        assert lib.mi355x_sd_freeu_workspace_floats(*args) == FB.workspace_floats(*args)
        sp = FB.launch(*args[:3], 5, args[3], False)
        assert args[0] * sp["splits"] * 7 * (args[3] + 14) <= FB.workspace_floats(*args)   # what the launch writes fits
    assert lib.mi355x_sd_freeu_workspace_floats(2, 1, 8, 8) == 0


REFUSED = {   # name -> changes to a valid call (cat, ld, B, H, W, Cx, Cs, b, s, elem_f32, workspace)
    "null cat": dict(cat=None), "null workspace": dict(workspace=None), "H < 2": dict(H=1), "W < 2": dict(W=1), "Cx < 0": dict(Cx=-1),
    "Cs < 1": dict(Cs=0), "ld < Cx + Cs": dict(ld=40), "misaligned cat": dict(cat=+2), "misaligned ld": dict(ld=52),
    "misaligned ld (fp32)": dict(ld=50, elem_f32=1), "b inf": dict(b=math.inf), "b nan": dict(b=math.nan), "s inf": dict(s=-math.inf),
    "s nan": dict(s=math.nan), "B < 1": dict(B=0),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_entry_refuses_before_the_device(what):
    lib = _lib.load()
    buf = torch.full((2 * 4 * 4 * 56,), 7.25, dtype=torch.float32)
    ws = torch.full((4096,), 7.25, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    call = dict(cat=buf.data_ptr(), ld=48, B=2, H=4, W=4, Cx=16, Cs=32, b=1.4, s=0.2, elem_f32=0, workspace=ws.data_ptr())
    for k, v in REFUSED[what].items():
        call[k] = call[k] + v if k == "cat" and v is not None else v
    rc = lib.mi355x_sd_freeu(call["cat"], call["ld"], call["B"], call["H"], call["W"], call["Cx"], call["Cs"], call["b"], call["s"],
                             call["elem_f32"], call["workspace"], None)
    assert rc == 1, (what, rc)
    assert lib.mi355x_sd_last_error().startswith(b"mi355x_sd_freeu:"), lib.mi355x_sd_last_error()
    assert bool((buf == 7.25).all()) and bool((ws == 7.25).all())


def test_handle_entry_refuses_a_null_handle_and_nonfinite_values():
    lib = _lib.load()
    assert lib.mi355x_sd_unet_set_freeu(None, 1, 0.9, 0.2, 1.3, 1.4) == 1
    assert lib.mi355x_sd_last_error().startswith(b"mi355x_sd_unet_set_freeu:")
    from paddlemix_amd.cexec import UNetHandle
    hd = UNetHandle(TINY)   # host side only: no device is touched before pack()
    good = (0.9, 0.2, 1.3, 1.4)
    for i in range(4):
        for bad in (math.nan, math.inf, -math.inf):
            args = list(good)
            args[i] = bad
            assert lib.mi355x_sd_unet_set_freeu(hd.h, 1, *args) == 1, (i, bad)
            assert b"must be finite" in lib.mi355x_sd_last_error()
    assert lib.mi355x_sd_unet_set_freeu(hd.h, 1, *good) == 0 and lib.mi355x_sd_unet_set_freeu(hd.h, 0, *good) == 0


# ---- the host logic on the emulator -------------------------------------------------------------------------------------------------
def _model(name, **kw):
    cfg, B, H, W, L = GEOM[name]
    P = synth_unet_params(cfg, seed=1234)
    Pb = {k: v.to(torch.bfloat16).float() if v.dim() > 1 else v for k, v in P.items()}
    emu = FreeUEmulator()
    return on_emulator(UNet2DConditionModel, cfg, P, backend=emu, **kw), emu, Pb, _inputs(cfg, B, H, W, L)


_ORACLE = {}


def _oracle(name, Pb, inputs, on):
    """the oracle's forward with / without FreeU, computed once per configuration and left unchanged"""
    if (name, on) not in _ORACLE:
        cfg = GEOM[name][0]
        sample, enc, added = inputs
        with pytest.MonkeyPatch.context() as mp:
            if on:
                FB.patch_oracle(mp, cfg, **FU)
            _ORACLE[(name, on)] = U.unet_forward(Pb, cfg, sample, 501, enc, added_cond_kwargs=added)
    return _ORACLE[(name, on)]


@pytest.mark.parametrize("name", list(GEOM))
@pytest.mark.parametrize("rd", [None, "fp32"])
def test_emulated_unet_with_freeu_matches_the_patched_oracle(name, rd):
    model, emu, Pb, (sample, enc, added) = _model(name, residual_dtype=rd)
    ref_on, ref_off = _oracle(name, Pb, (sample, enc, added), True), _oracle(name, Pb, (sample, enc, added), False)
    margin = _rel(ref_on, ref_off)
    assert margin >= 10 * TOL, margin            # FreeU moves the prediction by far more than the tolerance
    off = model(sample, 501, enc, added_cond_kwargs=added).sample
    assert "freeu" not in emu.calls
    model.enable_freeu(**FU)
    on = model(sample, 501, enc, added_cond_kwargs=added).sample
    print(f"{name} {rd}: on vs patched oracle {_rel(on, ref_on):.3e}, off vs oracle {_rel(off, ref_off):.3e}, margin {margin:.3f}")
    assert _rel(on, ref_on) < TOL and _rel(off, ref_off) < TOL
    assert all(c["elem_f32"] == (1 if rd else 0) for c in emu.freeu_calls)
    # (1, 1, 1, 1) and off-after-on are bit-identical to never on; every change of a constant plans again
    model.enable_freeu(1, 1, 1, 1)
    assert torch.equal(model(sample, 501, enc, added_cond_kwargs=added).sample, off) and len(model._plans) == 3
    model.disable_freeu()
    assert torch.equal(model(sample, 501, enc, added_cond_kwargs=added).sample, off) and len(model._plans) == 3
    model.enable_freeu(**dict(FU, b2=1.5))
    assert not torch.equal(model(sample, 501, enc, added_cond_kwargs=added).sample, on) and len(model._plans) == 4
    with pytest.raises(ValueError, match="finite"):
        model.enable_freeu(0.9, float("nan"), 1.3, 1.4)


@pytest.mark.parametrize("name", list(GEOM))
@pytest.mark.parametrize("controlnet", [False, True])
def test_plan_placement(name, controlnet):
    cfg, B, H, W, L = GEOM[name]
    model, emu, Pb, (sample, enc, added) = _model(name)
    model.enable_freeu(**FU)
    kw = {}
    if controlnet:   # residual shapes: every skip tensor, then the mid output
        ncfg, g = normalize_config(cfg), torch.Generator().manual_seed(5)
        shapes, h, w, c = [], H, W, ncfg["block_out_channels"][0]
        for d in _structure(ncfg, encoder_only=True):
            if d[0] == "resnet":
                c = d[3]
            elif d[0] == "down":
                h, w = (h + 1) // 2, (w + 1) // 2
            elif d[0] == "skip":
                shapes.append((B, c, h, w))
        kw = dict(down_block_additional_residuals=[0.1 * torch.randn(*s, generator=g) for s in shapes],
                  mid_block_additional_residual=0.1 * torch.randn(B, c, h, w, generator=g))
    model(sample, 501, enc, added_cond_kwargs=added, **kw)
    plan = list(model._plans.values())[-1]
    names = [fn.__name__ for fn, *_ in plan.prog]
    at = [i for i, n in enumerate(names) if n == "mi355x_sd_freeu"]
    ncfg = normalize_config(cfg)
    S, n = _structure(ncfg), len(ncfg["block_out_channels"])
    want = []   # (H, W, Cx, Cs, b, s) per up resnet of up blocks 0 and 1, in order
    for i, d in enumerate(S):
        if d[0] == "resnet" and d[1].startswith(("up_blocks.0.", "up_blocks.1.")):
            blk = int(d[1].split(".")[1])
            skip_c = S[i - 1][1]
            hw = H >> (n - 1 - blk)
            want.append((hw, hw, d[2] - skip_c, skip_c, FB.fp32(FU[f"b{blk + 1}"]), FB.fp32(FU[f"s{blk + 1}"])))
    lpb = ncfg["layers_per_block"]
    assert len(want) == (lpb[-1] + 1) + (lpb[-2] + 1) == len(at), (want, at)
    for i, w_ in zip(at, want):
        args = plan.prog[i][1]
        assert names[i + 1].startswith("mi355x_sd_groupnorm"), names[i:i + 2]     # directly before the resnet's first GroupNorm
        assert (args[3], args[4], args[5], args[6], FB.fp32(args[7]), FB.fp32(args[8])) == w_, (args, w_)
        assert args[2] == B and args[1] == w_[2] + w_[3] and args[9] == 0 and args[10]
    adds = [i for i, nm in enumerate(names) if nm.startswith("mi355x_sd_add_nchw")]
    assert bool(adds) == controlnet and all(i < at[0] for i in adds)             # after the ControlNet residual adds
    if name == "mini-xl":   # the third up block has none: nothing after the last launch but its own block's resnets and the rest
        last_hw = plan.prog[at[-1]][1][3]
        assert last_hw == H >> 1 and sum(1 for i in at if plan.prog[i][1][3] == H) == 0


@pytest.mark.parametrize("case", ["unet_tiny", "unet_mini_xl", "unet_tiny_masked_controlnet", "unet_tiny+resid_fp32"])
def test_off_after_on_is_the_recorded_plan(case, tmp_path):
    """enable_freeu, then disable_freeu: launch for launch and argument for argument what tests/golden/plan_tables.json recorded"""
    from paddlemix_amd.export import export_program
    from tests import plan_table_cases as PT
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_tables.json")))["cases"][case]
    model, run, outputs = on_emulator(PT.CASES[case], backend=FreeUEmulator())
    model.enable_freeu(**FU)
    model.disable_freeu()
    run()
    plans = list(model._plans.values())
    assert len(plans) == len(golden)
    for plan, g, i in zip(plans, golden, range(len(plans))):
        path = str(tmp_path / f"{i}.mi3prg")
        export_program(model, plan, path, outputs)
        assert [[fn.__name__, kind, fl] for fn, _, kind, fl in plan.prog] == g["prog"]
        assert PT.tables_digest(path) == g["tables_sha256"]


def test_controlnet_model_has_no_freeu():
    net = on_emulator(ControlNetModel, TINY, synth_controlnet_params(TINY, seed=3))
    with pytest.raises(ValueError, match="no up blocks"):
        net.enable_freeu(**FU)


def test_pipeline_forwards_to_the_unet():
    """a recorded loop with FreeU on differs from the loop with it off and equals the same loop driven by hand on a U-Net with FreeU"""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import DDIMScheduler
    sched = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, clip_sample=False, set_alpha_to_one=False)
    P = synth_unet_params(TINY, seed=1234)
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = torch.randn(1, 7, 64, generator=g), torch.randn(1, 7, 64, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    emu = FreeUEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, P, backend=emu), DDIMScheduler(**sched))
    run = lambda p: p(pe, ne, num_inference_steps=3, guidance_scale=5.0, latents=lat0.clone())  # noqa: E731
    off = run(pipe)
    assert not emu.freeu_calls
    pipe.enable_freeu(**FU)
    assert pipe.unet.freeu == tuple(FU[k] for k in ("s1", "s2", "b1", "b2"))
    on = run(pipe)
    assert len(emu.freeu_calls) == 3 * 6 and _rel(on, off) > 1e-2
    # the U-Net-level expectation: another pipeline around a U-Net that had FreeU enabled directly
    unet = on_emulator(UNet2DConditionModel, TINY, P, backend=FreeUEmulator())
    unet.enable_freeu(**FU)
    assert torch.equal(run(StableDiffusionDenoiser(unet, DDIMScheduler(**sched))), on)
    pipe.disable_freeu()
    assert pipe.unet.freeu is None and torch.equal(run(pipe), off)
