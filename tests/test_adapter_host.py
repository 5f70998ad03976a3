"""CPU tests of the T2I-Adapter (ABI 23): the torch restatement (tests/adapter_ref.py) against the outputs recorded from the reference's
own modules (tests/golden/adapter/), and the host logic -- adapter plan, intrablock adds in the U-Net plan, error paths, pipeline -- on
the emulator (tests/abi_emulator_adapter.py)."""
import os
import re

import pytest
import torch

from paddlemix_amd import _lib
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import adapter_cases as AC
from tests import adapter_ref as AR
from tests import reference_cases as RC
from tests.abi_emulator import Emulator, on_emulator
from tests.abi_emulator_adapter import AdapterEmulator

ROOT = AC.ROOT
TOL = 2e-2   # the emulated / device U-Net against the oracle on these small configurations (tests/test_host_logic.py, tests/test_gpu_unet.py)


def _max_rel(a, b):   # tests/test_reference_modules.py _rel, with its constant RC.REL_TOL
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ---- the restatement against the reference's recorded outputs -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AC.ADAPTER_GOLDEN))
def test_restatement_reproduces_the_reference_adapter(name):
    gold, config = AC.golden(f"adapter_{name}"), AR.ADAPTERS[name]
    B, H, W = AC.ADAPTER_GOLDEN[name]
    feats = AR.adapter_forward(AR.synth_adapter_params(config, seed=21), config, AC.image(B, config["in_channels"], H, W))
    assert len(feats) == sum(1 for k in gold.files if k.startswith("feature_"))
    for i, f in enumerate(feats):
        g = torch.from_numpy(gold[f"feature_{i}"])
        assert tuple(g.shape) == tuple(f.shape) and _max_rel(f, g) < RC.REL_TOL, (i, _max_rel(f, g))
    from paddlemix_amd.adapter import T2IAdapter
    net = on_emulator(T2IAdapter, config, AR.synth_adapter_params(config, seed=21), backend=AdapterEmulator())
    assert net.total_downscale_factor == int(gold["total_downscale_factor"]) and net.downscale_factor == int(gold["downscale_factor"])


def test_restatement_reproduces_the_reference_multi_adapter():
    gold, config = AC.golden("multi_adapter_full"), AR.ADAPTERS["full"]
    B, H, W = AC.ADAPTER_GOLDEN["full"]
    Ps = [AR.synth_adapter_params(config, seed=s) for s in (21, 22)]
    xs = [AC.image(B, 3, H, W, seed=s) for s in (11, 12)]
    for i, f in enumerate(AR.multi_adapter_forward(Ps, [config] * 2, xs, [0.7, 0.4])):
        assert _max_rel(f, torch.from_numpy(gold[f"feature_{i}"])) < RC.REL_TOL


@pytest.mark.parametrize("name", list(AC.UNET_GOLDEN))
def test_restatement_reproduces_the_reference_unet_forward(name):
    """every form the reference distinguishes: all sites, the deprecated argument, too few, the down blocks only, a surplus"""
    gold = AC.golden(f"unet_{name}")
    cfg, P, (sample, enc, added), res = AC.unet_golden_inputs(name)
    n_down = len(cfg["block_out_channels"])
    call = lambda **kw: AR.unet_forward_intrablock(P, cfg, sample, AC.T, enc, added_cond_kwargs=added, **kw)  # noqa: E731
    forms = AC.unet_golden_forms(res, n_down)
    got = {k: call(down_intrablock_additional_residuals=v) for k, v in forms.items()}
    got["deprecated"] = call(down_block_additional_residuals=forms["intrablock"])
    for k, v in got.items():
        assert _max_rel(v, torch.from_numpy(gold[k])) < RC.REL_TOL, (k, _max_rel(v, torch.from_numpy(gold[k])))
    g = {k: torch.from_numpy(gold[k]) for k in gold.files}
    # the recorded forms differ where the reference says they do, and only there
    assert torch.equal(g["deprecated"], g["intrablock"]) and torch.equal(g["surplus"], g["intrablock"])
    assert _rel(g["intrablock"], g["plain"]) > 5e-2 and _rel(g["too_few"], g["intrablock"]) > 1e-3
    if name == "xl":   # three down blocks: the fourth residual is the mid block's, and a fifth is ignored whatever its shape
        assert cfg["down_block_types"][0] == "DownBlock2D"   # ... and the first lands behind that block's downsampler
        assert _rel(g["down_only"], g["intrablock"]) > 1e-3 and torch.equal(g["mid_extra"], g["intrablock"])
    else:              # four down blocks take the four; a fifth of the mid output's shape is added after the mid block
        assert torch.equal(g["down_only"], g["intrablock"]) and _rel(g["mid_extra"], g["intrablock"]) > 1e-3


def test_restatement_pools_with_ceil_mode_and_exclusive_counts():
    x = torch.arange(2 * 1 * 3 * 5, dtype=torch.float64).reshape(2, 1, 3, 5)
    p = torch.nn.functional.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
    assert tuple(p.shape) == (2, 1, 2, 3) and p[0, 0, 1, 2] == x[0, 0, 2, 4] and p[0, 0, 0, 2] == (x[0, 0, 0, 4] + x[0, 0, 1, 4]) / 2
    assert AR.intrablock_shapes(AC.MINI_SD15, 1, 9, 11) == [(1, 64, 9, 11), (1, 128, 5, 6), (1, 256, 3, 3), (1, 256, 2, 2), (1, 256, 2, 2)]
    assert AR.intrablock_shapes(AC.UNETS["xl"][0], 1, 18, 22) == [(1, 64, 9, 11), (1, 128, 9, 11), (1, 256, 5, 6), (1, 256, 5, 6)]


# ---- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_abi():
    hdr = open(os.path.join(ROOT, "include", "mi355x_sd.h")).read()
    for sym in ("mi355x_sd_pixel_unshuffle", "mi355x_sd_avgpool2", "mi355x_sd_relu"):
        assert f" {sym}(" in hdr and sym in _lib.SIGNATURES
    abi = int(re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION >= 23
    assert _lib.load().mi355x_sd_abi_version() == abi


REFUSED = [   # (entry, arguments after the pointers are filled in, what is wrong); every one returns before the device is touched
    ("unshuffle", dict(x=None), 1), ("unshuffle", dict(y=None), 1), ("unshuffle", dict(H=20), 1), ("unshuffle", dict(W=12), 1),
    ("unshuffle", dict(ldy=184), 1), ("unshuffle", dict(ldy=196), 1), ("unshuffle", dict(r=0), 1),
    ("avgpool", dict(x=None), 1), ("avgpool", dict(ldx=8), 1), ("avgpool", dict(ldy=8), 1), ("avgpool", dict(C=12, ldx=16, ldy=16), 2),
    ("avgpool", dict(ldx=20), 2), ("avgpool", dict(H=0), 1),
    ("relu", dict(x=None), 1), ("relu", dict(rows=0), 1), ("relu", dict(ldx=8), 1),
]


@pytest.mark.parametrize("entry,change,want", REFUSED)
def test_entries_refuse_before_the_device(entry, change, want):
    lib = _lib.load()
    buf = torch.full((4096,), 7.25, dtype=torch.float32)
    out = torch.full((4096,), 7.25, dtype=torch.float32)
    if entry == "unshuffle":
        a = dict(x=buf.data_ptr(), B=1, C=3, H=16, W=16, r=8, y=out.data_ptr(), ldy=192)
        a.update(change)
        rc = lib.mi355x_sd_pixel_unshuffle(a["x"], a["B"], a["C"], a["H"], a["W"], a["r"], a["y"], a["ldy"], None)
    elif entry == "avgpool":
        a = dict(x=buf.data_ptr(), ldx=16, B=1, H=3, W=3, C=16, y=out.data_ptr(), ldy=16)
        a.update(change)
        rc = lib.mi355x_sd_avgpool2(a["x"], a["ldx"], a["B"], a["H"], a["W"], a["C"], a["y"], a["ldy"], None)
    else:
        a = dict(x=buf.data_ptr(), ldx=16, y=out.data_ptr(), ldy=16, rows=4, C=16)
        a.update(change)
        rc = lib.mi355x_sd_relu(a["x"], a["ldx"], a["y"], a["ldy"], a["rows"], a["C"], None)
    assert rc == want, (entry, change, rc)
    assert lib.mi355x_sd_last_error().startswith(b"mi355x_sd_"), lib.mi355x_sd_last_error()
    assert bool((buf == 7.25).all()) and bool((out == 7.25).all())


# ---- the adapter on the emulator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,W", [("full", 64, 64), ("full", 72, 88), ("xl", 64, 64), ("xl-r8", 72, 88), ("light", 64, 64), ("light", 72, 88)])
def test_emulated_adapter_matches_the_restatement(name, H, W):
    from paddlemix_amd.adapter import T2IAdapter
    config = dict(AR.ADAPTERS["xl"], downscale_factor=8) if name == "xl-r8" else AR.ADAPTERS[name]
    P = AR.synth_adapter_params(config, seed=21)
    emu = AdapterEmulator()
    net = on_emulator(T2IAdapter, config, P, backend=emu)
    x = AC.image(2, config["in_channels"], H, W)
    feats = net(x)
    ref = AR.adapter_forward(AC.rounded(P), config, x)
    assert len(feats) == len(ref)
    for f, r in zip(feats, ref):
        assert f.dtype == torch.float32 and tuple(f.shape) == tuple(r.shape) and _rel(f, r) < TOL, (_rel(f, r), f.shape)
    assert emu.calls.count("pixel_unshuffle") == 1 and emu.calls.count("relu") == len(ref) * config["num_res_blocks"]
    assert emu.calls.count("avgpool2") == sum(1 for _, _, d in AR._blocks(AR.normalize_adapter_config(config)) if d)
    assert all(torch.equal(a, b) for a, b in zip(net(x), feats)) and len(net._plans) == 1
    if (H, W) == (72, 88) and name == "full":   # every pool is a ceil-mode one and the sizes are the U-Net's own
        assert [tuple(f.shape) for f in feats] == AR.intrablock_shapes(AC.MINI_SD15, 2, 9, 11)[:4]


def test_adapter_error_paths_and_multi_adapter():
    from paddlemix_amd.adapter import MultiAdapter, T2IAdapter
    import paddlemix_amd
    assert paddlemix_amd.T2IAdapter is T2IAdapter and paddlemix_amd.MultiAdapter is MultiAdapter
    config = AR.ADAPTERS["full"]
    Ps = [AR.synth_adapter_params(config, seed=s) for s in (21, 22)]
    a, b = (on_emulator(T2IAdapter, config, P, backend=AdapterEmulator()) for P in Ps)
    with pytest.raises(ValueError, match="multiples of downscale_factor"):
        a(AC.image(1, 3, 60, 64))
    with pytest.raises(ValueError, match="expected an image"):
        a(AC.image(1, 1, 64, 64))
    for bad in (dict(config, channels=(60, 128)), dict(config, in_channels=1, downscale_factor=2), dict(AR.ADAPTERS["light"], channels=(72, 144))):
        with pytest.raises(ValueError, match="multiple"):
            on_emulator(T2IAdapter, bad, {}, backend=AdapterEmulator())
    with pytest.raises(ValueError, match="Unsupported adapter_type"):
        on_emulator(T2IAdapter, dict(config, adapter_type="heavy"), {}, backend=AdapterEmulator())
    with pytest.raises(KeyError, match="missing parameters"):
        on_emulator(T2IAdapter, config, {}, backend=AdapterEmulator())
    # MultiAdapter: the reference's checks, the weighted sum, both input forms
    with pytest.raises(ValueError, match="at least one"):
        MultiAdapter([])
    with pytest.raises(ValueError, match="single adapter"):
        MultiAdapter([a])
    other = dict(config, downscale_factor=16)
    c = on_emulator(T2IAdapter, other, AR.synth_adapter_params(other, seed=3), backend=AdapterEmulator())
    with pytest.raises(ValueError, match="same downscaling behavior"):
        MultiAdapter([a, c])
    multi = MultiAdapter([a, b])
    assert (multi.downscale_factor, multi.total_downscale_factor) == (8, 64)
    xs = [AC.image(2, 3, 64, 64, seed=s) for s in (11, 12)]
    got = multi(xs, [0.7, 0.4])
    ref = AR.multi_adapter_forward([AC.rounded(P) for P in Ps], [config] * 2, xs, [0.7, 0.4])
    assert all(_rel(g, r) < TOL for g, r in zip(got, ref))
    assert all(torch.equal(g, h) for g, h in zip(multi(torch.cat(xs, 1), [0.7, 0.4]), got))     # the channel-concatenated form
    half = multi(xs)
    assert all(torch.equal(h, 0.5 * fa + 0.5 * fb) for h, fa, fb in zip(half, a(xs[0]), b(xs[1])))
    with pytest.raises(ValueError, match="adapters"):
        multi(xs[:1])


# ---- the intrablock adds in the U-Net plan --------------------------------------------------------------------------------------------
def _unet(name, **kw):
    cfg, _, _, L = AC.UNETS[name]
    P = synth_unet_params(cfg, seed=1234)
    emu = AdapterEmulator()
    return on_emulator(UNet2DConditionModel, cfg, P, backend=emu, **kw), emu, AC.rounded(P), cfg, L


def _prog(plan):
    return [(fn.__name__, kind, fl) for fn, _, kind, fl in plan.prog]


@pytest.mark.parametrize("name", list(AC.UNETS))
def test_no_residuals_leaves_the_plan_as_it_is(name):
    """(a) the plain plan of a model that has planned intrablock adds equals, launch for launch and key for key, the plan a model
    builds that never saw an adapter argument"""
    cfg, _, _, L = AC.UNETS[name]
    P = synth_unet_params(cfg, seed=1234)
    sample, enc, added = AC.unet_inputs(cfg, 2, 16, 16, L)
    fresh = on_emulator(UNet2DConditionModel, cfg, P, backend=Emulator())
    plain = fresh(sample, AC.T, enc, added_cond_kwargs=added).sample
    before = {k: _prog(p) for k, p in fresh._plans.items()}
    model, emu, _, _, _ = _unet(name)
    res = AC.residuals(cfg, 2, 16, 16)
    model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=res)
    assert "add_nchw" in emu.calls
    n = len(emu.calls)
    out = model(sample, AC.T, enc, added_cond_kwargs=added).sample
    assert "add_nchw" not in emu.calls[n:] and torch.equal(out, plain)
    keys = list(model._plans)
    assert len(keys) == 2 and keys[1] in before and keys[0] == keys[1] + (len(res),)       # the key gains the count, and only with residuals
    assert _prog(model._plans[keys[1]]) == before[keys[1]]
    assert [len(t) for t in (model._plans[keys[1]].keep, fresh._plans[keys[1]].keep)] == [len(fresh._plans[keys[1]].keep)] * 2
    assert not model._plans[keys[1]].intra and len(model._plans[keys[0]].intra) == len(res)
    # the same through an explicit None and an empty list
    assert torch.equal(model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=None).sample, plain)
    assert torch.equal(model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=[]).sample, plain)
    assert len(model._plans) == 2


OUT_ARG = {"mi355x_sd_conv3x3": 9, "mi355x_sd_linear": 3}   # where a producer's output pointer sits among its arguments


@pytest.mark.parametrize("name", list(AC.UNETS))
@pytest.mark.parametrize("rd", [None, "fp32"])
def test_each_add_sits_behind_its_producer_and_matches_the_restatement(name, rd):
    """(b) four adds (the XL shape's fourth is the mid block's), each directly behind the launch that writes the tensor and before
    the first launch that reads it; (c) the deprecated form is the same plan; the forward matches the restatement"""
    model, emu, Pb, cfg, L = _unet(name, residual_dtype=rd)
    B, H, W = 2, 16, 16
    sample, enc, added = AC.unet_inputs(cfg, B, H, W, L)
    res = AC.residuals(cfg, B, H, W)
    out = model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=[r.clone() for r in res]).sample
    plan = list(model._plans.values())[-1]
    names = [fn.__name__ for fn, *_ in plan.prog]
    adds = [i for i, n in enumerate(names) if n.startswith("mi355x_sd_add_nchw")]
    shapes = AR.intrablock_shapes(cfg, B, H, W)
    assert len(adds) == 4 == len(plan.intra) and [tuple(t.shape) for t in plan.intra] == shapes[:4]
    producers = []
    for i, t in zip(adds, plan.intra):
        args, prev = plan.prog[i][1], plan.prog[i - 1]
        assert names[i] == ("mi355x_sd_add_nchw_ex" if rd else "mi355x_sd_add_nchw") and args[2] == t.data_ptr()
        assert (args[3], args[4], args[5]) == (B, t.shape[1], t.shape[2] * t.shape[3])
        assert names[i - 1] in OUT_ARG and prev[1][OUT_ARG[names[i - 1]]] == args[0], (names[i - 1], "writes another tensor")
        producers.append(names[i - 1] + (":s2" if names[i - 1] == "mi355x_sd_conv3x3" and prev[1][6] == 2 else ""))
        # ... and nothing before the producer reads or writes that address in this block: the next launch is the first consumer
        assert not names[i + 1].startswith("mi355x_sd_add_nchw")
    if name == "sd15":   # three attention blocks (proj_out), then the last DownBlock2D's resnet (conv2): no add behind a downsampler
        assert producers == ["mi355x_sd_linear"] * 3 + ["mi355x_sd_conv3x3"]
    else:                # the DownBlock2D's downsampler (stride 2), two attention blocks, the mid block's last resnet
        assert producers == ["mi355x_sd_conv3x3:s2", "mi355x_sd_linear", "mi355x_sd_linear", "mi355x_sd_conv3x3"]
    ref = AR.unet_forward_intrablock(Pb, cfg, sample, AC.T, enc, down_intrablock_additional_residuals=res, added_cond_kwargs=added)
    plain = model(sample, AC.T, enc, added_cond_kwargs=added).sample
    assert _rel(out, ref) < TOL and _rel(out, plain) > 5e-2, (_rel(out, ref), _rel(out, plain))
    # (c) the deprecated form: the same plan object, the same bits
    dep = model(sample, AC.T, enc, added_cond_kwargs=added, down_block_additional_residuals=res).sample
    assert torch.equal(dep, out) and len(model._plans) == 2
    # zero residuals: x + 0 is exact
    zero = model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=[torch.zeros_like(r) for r in res]).sample
    assert torch.equal(zero, plain)
    assert len(res) == 4   # the caller's list is not consumed


def test_too_few_too_many_and_the_mid_rule():
    model, emu, Pb, cfg, L = _unet("xl")
    B, H, W = 2, 16, 16
    sample, enc, added = AC.unet_inputs(cfg, B, H, W, L)
    res = AC.residuals(cfg, B, H, W, extra=1)
    call = lambda r: model(sample, AC.T, enc, added_cond_kwargs=added, down_intrablock_additional_residuals=r).sample  # noqa: E731
    ref = lambda r: AR.unet_forward_intrablock(Pb, cfg, sample, AC.T, enc, down_intrablock_additional_residuals=r, added_cond_kwargs=added)  # noqa: E731
    full = call(res[:4])
    assert torch.equal(call(res), full)                                   # a surplus residual is ignored
    few = call(res[:2])
    assert _rel(few, ref(res[:2])) < TOL and _rel(few, full) > 1e-3       # only the first blocks get one
    wrong_mid = res[:3] + [torch.zeros(B, 256, 3, 3)]
    down_only = call(wrong_mid)                                            # a left-over of another shape is not the mid block's
    assert torch.equal(down_only, call(res[:3])) and _rel(down_only, ref(res[:3])) < TOL
    assert sorted(k[-1] for k in model._plans if len(k) == 10) == [2, 3, 4]
    with pytest.raises(ValueError, match=r"down_intrablock_additional_residuals\[1\]"):
        call([res[0], res[0]])


# ---- (d) error paths ------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    from paddlemix_amd.cexec import CUNet2DConditionModel
    model, emu, Pb, cfg, L = _unet("sd15")
    B, H, W = 2, 16, 16
    sample, enc, added = AC.unet_inputs(cfg, B, H, W, L)
    res = AC.residuals(cfg, B, H, W)
    skips = [torch.zeros(B, 64, 16, 16)] * 3
    with pytest.raises(NotImplementedError, match="together with ControlNet"):
        model(sample, AC.T, enc, down_intrablock_additional_residuals=res, down_block_additional_residuals=skips,
              mid_block_additional_residual=torch.zeros(B, 256, 2, 2))
    with pytest.raises(NotImplementedError, match="both"):   # ControlNet-shaped down residuals without the mid one: no adapter's shapes
        model(sample, AC.T, enc, down_block_additional_residuals=[torch.zeros(B, 64, 16, 16), torch.zeros(B, 64, 16, 16)])
    # the C executor refuses the adapter form by name, before it touches a device
    c = CUNet2DConditionModel.__new__(CUNet2DConditionModel)
    c.hd = type("H", (), dict(lib=None, h=None, config_dict=dict(cfg)))()
    for kw in (dict(down_intrablock_additional_residuals=res), dict(down_block_additional_residuals=res)):
        with pytest.raises(NotImplementedError, match="T2I-Adapter"):
            CUNet2DConditionModel.forward(c, sample, AC.T, enc, **kw)


# ---- (f) the pipeline -----------------------------------------------------------------------------------------------------------------
class _SpyUNet:
    """the U-Net as the pipeline sees it, with the intrablock argument of every call recorded"""

    def __init__(self, unet):
        self.unet, self.config, self._lib, self._emulated = unet, unet.config, unet._lib, unet._emulated
        self.seen, self.lists = [], []

    def __call__(self, *a, **k):
        r = k.get("down_intrablock_additional_residuals")
        self.seen.append(None if r is None else [tuple(t.shape) for t in r])
        self.lists.append(r)
        return self.unet(*a, **k)


class _Counting:
    def __init__(self, adapter):
        self.adapter, self.calls = adapter, 0
        self.downscale_factor, self.total_downscale_factor = adapter.downscale_factor, adapter.total_downscale_factor

    def __call__(self, x):
        self.calls += 1
        return self.adapter(x)


def test_pipeline_runs_the_adapter_once_and_withholds_by_factor():
    from paddlemix_amd.adapter import T2IAdapter
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.schedulers import DDIMScheduler
    sched = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, clip_sample=False, set_alpha_to_one=False)
    cfg = AC.MINI_SD15
    emu = AdapterEmulator()
    unet = spy = _SpyUNet(on_emulator(UNet2DConditionModel, cfg, synth_unet_params(cfg, seed=1234), backend=emu))
    seen = spy.seen
    config = AR.ADAPTERS["full"]
    adapter = _Counting(on_emulator(T2IAdapter, config, AR.synth_adapter_params(config, seed=21), backend=AdapterEmulator()))
    pipe = StableDiffusionDenoiser(unet, DDIMScheduler(**sched), adapter=adapter)
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = torch.randn(1, 7, 64, generator=g), torch.randn(1, 7, 64, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    img = AC.image(1, 3, 70, 64)   # floored to 64 x 64 -> 8 x 8 latents
    run = lambda **kw: pipe(pe, ne, num_inference_steps=4, guidance_scale=5.0, latents=lat0.clone(), **kw)  # noqa: E731
    plain = run()
    assert adapter.calls == 0 and seen == [None] * 4
    del seen[:], spy.lists[:]
    on = run(adapter_image=img)
    assert adapter.calls == 1 and all(s == AR.intrablock_shapes(cfg, 2, 8, 8)[:4] for s in seen) and len(seen) == 4
    assert len({id(r) for r in spy.lists}) == 4                       # a fresh list every step
    assert torch.isfinite(on).all() and _rel(on, plain) > 1e-2
    del seen[:]
    half = run(adapter_image=img, adapter_conditioning_factor=0.6)   # int(4 * 0.6) = 2: steps 0 and 1 only
    assert adapter.calls == 2 and [s is not None for s in seen] == [True, True, False, False]
    assert not torch.equal(half, on) and not torch.equal(half, plain)
    del seen[:]
    assert torch.equal(run(adapter_image=img, adapter_conditioning_factor=0.0), plain) and seen == [None] * 4
    assert torch.equal(run(adapter_image=img, adapter_conditioning_scale=0.0), plain)       # x + 0
    scaled = run(adapter_image=img, adapter_conditioning_scale=0.5)
    assert not torch.equal(scaled, on) and not torch.equal(scaled, plain)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        run(adapter_image=img, control_image=torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="needs an `adapter`"):
        StableDiffusionDenoiser(unet, DDIMScheduler(**sched))(pe, ne, num_inference_steps=2, latents=lat0.clone(), adapter_image=img)
