"""CPU tests of the panorama loop (ABI 26): the recorded loops of the reference's own pipeline against the restatement
(tests/panorama_ref.py), the loop of StableDiffusionDenoiser(panorama=True) on the emulated device (tests/abi_emulator_panorama.py)
against the restatement and the record, fused_views and view_batch_size leaving the bits alone, the emulator's two passes against the
reference's expressions on the kernel matrix, the view table, the U-Net batch, the host and entry refusals, the unchanged text2img
loop and the padded decode.

Tolerances, stated before any run. Restatement against record, and the emulated loop against both: LOOP_TOL = 2^-14 of the largest
latent, what tests/test_sega_host.py holds the same kind of pair to around the same stand-in U-Net (float32 loops of a few dozen
operations per element and step that differ in the order of their roundings). With ``fused_update=False`` the loop runs the
restatement's own operations around exact view passes, so there it is held to EQUAL BITS. With the fused Heun tail the bar is the one
tests/test_fused_heun.py states for that tail against ``scheduler.step`` in float32, 2^-9 of the largest latent: the reference's Heun
step forms (x - (x - sigma e)) / sigma, the tail its coefficient form, and a plain text2img loop around this stand-in differs by
1.1e-4 between the two at 4 steps (7 evaluations) -- the view passes add nothing to that, which the equal bits of the generic path
and of fused_views show.

The guided batch-2 record (``pndm_two_rows``) is NOT what this loop computes, and that is asserted: the reference interleaves the
latents ``[x0, x0, x1, x1]`` against embeddings tiled ``[neg0, neg1, text0, text1]``, so even with one prompt repeated image 0 is
denoised with the negative prompt in BOTH guidance halves and image 1 with the text prompt in both -- no guidance at all. The
restatement reproduces that record; the denoiser pairs every image with its own two prompts and is held, per image, to the
restatement at batch 1."""
import os
import re
from ctypes import c_float, c_int, c_int64, c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from paddlemix_amd import _lib, ops
from paddlemix_amd import panorama_forms as PF
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import configs
from tests import panorama_cases as C
from tests import panorama_ref as R
from tests.abi_emulator import on_emulator
from tests.abi_emulator_panorama import ENTRIES, PanoramaEmulator, refused, view_input_math, view_merge_math
from tests.header_decls import declared

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "panorama", "loops.npz"))
LOOP_TOL = 2.0 ** -14
HEUN_TOL = 2.0 ** -9    # tests/test_fused_heun.py test_routing_around_the_heun_entry


def _config():
    return SimpleNamespace(time_cond_proj_dim=None, addition_embed_type=None, sample_size=64, in_channels=4)


def _formula():
    f, emu = C.FormulaUNet(_config()), PanoramaEmulator()
    f._lib, f._emulated = emu, True
    return f, emu


def _case(name):
    sched, shape_name, gs = C.GOLDEN[name]
    shape, circular, vbs = C.SHAPES[shape_name]
    return sched, gs, circular, vbs, C.loop_inputs(shape)


def bits_off(a, b):
    return int(((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)) & ~(torch.isnan(a) & torch.isnan(b))).sum())


@pytest.fixture(scope="module")
def restated():
    """the restatement's end latents of every recorded loop, computed once"""
    out = {}
    for name in C.GOLDEN:
        sched, gs, circular, vbs, (pe, ne, lat) = _case(name)
        out[name] = R.loop(C.FormulaUNet(_config()), C.SCHEDULERS[sched](), pe, ne, lat, C.STEPS, gs, vbs, circular)
    return out


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_restatement_against_the_references_own_pipeline(name, restated):
    gold, want = torch.from_numpy(GOLD[name]), restated[name]
    tol = LOOP_TOL * float(gold.abs().max())
    print(f"{name}: |restatement - reference| {float((want - gold).abs().max()):.2e} of {float(gold.abs().max()):.1f} (tolerance {tol:.2e})")
    assert torch.isfinite(gold).all() and float((want - gold).abs().max()) < tol
    if "two_rows" in name:
        assert int((gold == 0).sum()) == 2304 and bool((gold[..., 72:] == 0).all())      # the four columns no view covers


@pytest.mark.parametrize("fused_update", [True, False])
@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_denoiser_loop_on_the_emulator_against_the_restatement_and_the_record(name, fused_update, restated):
    sched, gs, circular, vbs, (pe, ne, lat) = _case(name)
    formula, emu = _formula()
    pipe = StableDiffusionDenoiser(formula, C.SCHEDULERS[sched]())
    kw = dict(num_inference_steps=C.STEPS, guidance_scale=gs, latents=lat.clone(), panorama=True, circular_padding=circular,
              fused_update=fused_update)
    got = pipe(pe, ne, view_batch_size=vbs, **kw)
    iters, total = len(pipe.scheduler.timesteps), len(PF.views(*lat.shape[2:], circular=circular))
    chunks = -(-total // vbs)
    assert emu.calls.count("view_merge") == iters and emu.calls.count("view_input") >= iters * chunks
    assert {c["groups"] for c in emu.view_input_calls} <= {1, 2 if gs > 1.0 else 1}
    gold, want = torch.from_numpy(GOLD[name]), restated[name]
    if lat.shape[0] > 1 and gs > 1.0:
        # the documented departure (module docstring): own prompts per image, the restatement at batch 1 per image
        assert float((got - gold).abs().max()) > 0.1 * float(gold.abs().max())
        want = torch.cat([R.loop(formula, C.SCHEDULERS[sched](), pe[b:b + 1], ne[b:b + 1], lat[b:b + 1], C.STEPS, gs, vbs, circular)
                          for b in range(lat.shape[0])])
        gold = want
    tol = (HEUN_TOL if sched == "heun" and fused_update else LOOP_TOL) * float(want.abs().max())
    print(f"{name} fused_update={fused_update}: |loop - restatement| {float((got - want).abs().max()):.2e} |loop - record| "
          f"{float((got - gold).abs().max()):.2e} of {float(want.abs().max()):.1f} (tolerance {tol:.2e})")
    assert float((got - want).abs().max()) < tol and float((got - gold).abs().max()) < tol
    if not fused_update:
        assert bits_off(got, want) == 0                      # scheduler.step around exact view passes: the restatement's own bits
    # fused_views=False: the same step in torch ops, equal bits, and no launch of the two entries
    n_in, n_merge = emu.calls.count("view_input"), emu.calls.count("view_merge")
    assert bits_off(pipe(pe, ne, view_batch_size=vbs, fused_views=False, **kw), got) == 0
    assert (emu.calls.count("view_input"), emu.calls.count("view_merge")) == (n_in, n_merge)
    if fused_update:                                         # chunking: 1, 3 and all views per U-Net call give equal bits
        for other in (1, 3, None):
            if other != vbs:
                assert bits_off(pipe(pe, ne, view_batch_size=other, **kw), got) == 0, other


@pytest.mark.parametrize("name", list(C.KERNEL))
def test_emulators_passes_are_the_references_expressions_bit_for_bit(name):
    spec = C.KERNEL[name]
    x, views = C.kernel_inputs(spec, seed=sorted(C.KERNEL).index(name))
    geo = [spec[k] for k in ("win_h", "win_w", "stride", "ny", "nx", "circular")]
    for groups in (1, 2):
        ref = R.kernel_reference(spec, x, views, C.SCALE, groups)
        got = view_input_math(x, C.SCALE, groups, *geo, ref["first"], ref["n"])
        assert bits_off(got.reshape(ref["input"].shape), ref["input"]) == 0
    merged = view_merge_math(views, spec["batch"], spec["C"], spec["H"], spec["W"], *geo)
    assert bits_off(merged, ref["merged"]) == 0
    assert merged[0, 0, 0, 1].view(torch.int32).item() == 0 and ref["count"][0, 0, 0, 1] > 0      # every covering view holds -0.0: +0.0
    assert bool((merged[ref["count"] == 0].view(torch.int32) == 0).all())
    assert ref["recip"] > 0 or not ref["odd_counts"]        # a reciprocal multiply would show wherever a count is no power of two
    assert torch.isnan(merged).sum() == 1 and torch.isinf(merged).sum() == 2


def test_the_matrix_holds_counts_a_reciprocal_would_miss():
    odd = [n for n, s in C.KERNEL.items() if R.kernel_reference(s, *C.kernel_inputs(s, 0), 1.0, 1)["odd_counts"]]
    assert any("w8s1" in n for n in odd) and any("w64s8 64x80 b" in n for n in odd)


@pytest.mark.parametrize("size, circular, want", [((512, 2048), False, 25), ((512, 2048), True, 32), ((512, 640), True, 10),
                                                   ((576, 608), False, 4), ((1024, 1024), False, 81), ((512, 512), True, 1),
                                                   ((256, 2048), False, 25), ((520, 700), False, 3)])
def test_view_table_is_the_references_get_views(size, circular, want):
    h, w = size[0] // 8, size[1] // 8
    table = R.get_views(*size, circular_padding=circular)
    assert PF.views(h, w, circular=circular) == table and len(table) == want
    ny, nx, wh, ww = PF.grid(h, w, circular=circular)
    assert ny * nx == want and (wh, ww) == (min(h, 64), min(w, 64))


def test_unet_batch_is_negative_times_views_then_text_times_views():
    pe, ne, lat = C.loop_inputs((2, 4, 64, 80))
    pe, ne = pe + torch.arange(2.0).reshape(2, 1, 1), ne - torch.arange(2.0).reshape(2, 1, 1)     # every image its own two prompts
    seen = []

    class Spy(C.FormulaUNet):
        def __call__(self, x, t, encoder_hidden_states=None, **kw):
            seen.append((x.clone(), encoder_hidden_states))
            return super().__call__(x, t, encoder_hidden_states=encoder_hidden_states, **kw)
    spy = Spy(_config())
    spy._lib, spy._emulated = PanoramaEmulator(), True
    StableDiffusionDenoiser(spy, C.SCHEDULERS["euler"]())(pe, ne, num_inference_steps=1, latents=lat.clone(), panorama=True)
    (x, enc), = seen
    assert torch.equal(enc, torch.cat([ne.repeat(3, 1, 1), pe.repeat(3, 1, 1)])) and x.shape == (12, 4, 64, 64)
    assert torch.equal(x[:6], x[6:])                          # equal planes in both groups
    sch = C.SCHEDULERS["euler"]()
    sch.set_timesteps(1)
    scaled = sch.scale_model_input(lat * sch.init_noise_sigma, sch.timesteps[0])
    assert torch.allclose(x[2:4], scaled[:, :, :, 8:72], rtol=1e-6, atol=0)                       # sample v * B + b: view 1 of both images


def test_host_refusals_each_by_name():
    pe, ne, lat = C.loop_inputs((1, 4, 64, 80))
    kw = dict(num_inference_steps=1, latents=lat.clone(), panorama=True)

    def pipe(sched, unet=None):
        return StableDiffusionDenoiser(unet or _formula()[0], sched)
    noisy = {"euler_a": C.S.EulerAncestralDiscreteScheduler(**C.SCHED), "dpm2_a": C.S.KDPM2AncestralDiscreteScheduler(**C.SCHED)}
    for sch in noisy.values():
        with pytest.raises(NotImplementedError, match="draws noise"):
            pipe(sch)(pe, ne, **kw)
    with pytest.raises(NotImplementedError, match="draws noise.*eta > 0"):
        pipe(C.SCHEDULERS["ddim"]())(pe, ne, eta=0.5, **kw)
    tall = C.loop_inputs((1, 4, 72, 80))[2]
    with pytest.raises(NotImplementedError, match="more than one row of views"):
        pipe(C.SCHEDULERS["ddim"]())(pe, ne, circular_padding=True, **dict(kw, latents=tall))
    plane = torch.zeros(1, 1, 8, 8)
    for name, v in (("guidance_rescale", 0.7), ("image_guidance_scale", 1.5), ("image", plane), ("mask_image", plane),
                    ("control_image", plane), ("adapter_image", plane), ("added_cond_kwargs", {"text_embeds": plane}),
                    ("editing_prompt_embeds", pe), ("editing_prompt_ids", torch.zeros(1, 7, dtype=torch.long))):
        with pytest.raises(NotImplementedError, match=f"`{name}` together with `panorama`"):
            pipe(C.SCHEDULERS["ddim"]())(pe, ne, **kw, **{name: v})
    for attr, value, match in (("addition_embed_type", "text_time", "addition_embed_type"), ("time_cond_proj_dim", 32, "time_cond_proj_dim")):
        unet = _formula()[0]
        setattr(unet.config, attr, value)
        with pytest.raises(NotImplementedError, match=match):
            pipe(C.SCHEDULERS["ddim"](), unet)(pe, ne, **kw)
    with pytest.raises(ValueError, match="view_batch_size"):
        pipe(C.SCHEDULERS["ddim"]())(pe, ne, view_batch_size=0, **kw)


def test_text2img_calls_and_bits_are_unchanged_without_panorama():
    cfg = configs.TINY
    g = torch.Generator().manual_seed(5)
    pe, ne = (torch.randn(1, C.TOKENS, cfg["cross_attention_dim"], generator=g) for _ in range(2))
    lat = torch.randn(1, 4, 8, 8, generator=g)
    emu = PanoramaEmulator()
    unet = on_emulator(UNet2DConditionModel, cfg, synth_unet_params(cfg, seed=1), backend=emu)
    pipe = StableDiffusionDenoiser(unet, C.SCHEDULERS["euler"]())

    def text2img(**kw):
        emu.calls.clear()
        return pipe(pe, ne, num_inference_steps=2, guidance_scale=C.GS, latents=lat.clone(), **kw), list(emu.calls)
    a, calls_a = text2img()
    assert "view_input" not in calls_a and "view_merge" not in calls_a
    emu.calls.clear()
    pano = pipe(pe, ne, num_inference_steps=2, guidance_scale=C.GS, latents=lat.clone(), panorama=True)
    assert emu.calls.count("view_merge") == 2 and pano.shape == a.shape
    b, calls_b = text2img(view_batch_size=3, circular_padding=True, fused_views=False)            # ignored without `panorama`
    assert calls_a == calls_b and torch.equal(a, b)


def test_padded_decode_is_the_decode_of_the_padded_latents_cropped():
    class Vae:
        config = SimpleNamespace(scaling_factor=0.5)

        def decode(self, z, return_dict=False, in_scale=1.0):
            up = (z * in_scale).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
            return (up[:, :3] + 0.01 * torch.arange(up.shape[3]),)                                # depends on the pixel column
    pipe = StableDiffusionDenoiser(_formula()[0], C.SCHEDULERS["ddim"](), vae=Vae())
    lat = torch.randn(1, 4, 8, 24, generator=torch.Generator().manual_seed(2)) * 0.3
    padded = torch.cat((lat[..., -8:], lat, lat[..., :8]), dim=-1)
    want = pipe.decode_latents(padded)[..., 64:-64]
    got = pipe.decode_latents(lat, circular_padding=True)
    assert got.shape == (1, 3, 64, 192) and torch.equal(got, want) and not torch.equal(got, pipe.decode_latents(lat))
    assert pipe.decode_latents(lat, "np", circular_padding=True).shape == (1, 64, 192, 3)


# ---------------------------------------------------------------------------------------------------- header, binding, refusals
CTYPES = {"const float*": c_void_p, "float*": c_void_p, "void*": c_void_p, "int": c_int, "float": c_float, "int64_t": c_int64}


@pytest.mark.parametrize("entry", list(ENTRIES.values()), ids=list(ENTRIES))
def test_entry_is_its_declaration_in_the_header(entry):
    ret, params = declared()["mi355x_sd_" + entry.entry]
    assert ret == "int" and params == [tuple(p) for p in entry.params]
    assert all((kind == "float*") == (n in entry.written) for kind, n in params if kind.endswith("float*"))
    restype, argtypes = _lib.SIGNATURES["mi355x_sd_" + entry.entry]
    assert restype is c_int and list(argtypes) == [CTYPES[kind] for kind, _ in params]
    assert set(entry.spans) == {n for kind, n in params if kind.endswith("float*")} and callable(getattr(ops, entry.entry))


def test_abi_version_26_in_header_binding_and_library():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mi355x_sd.h")).read()
    abi = int(re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION == 26
    assert _lib.load().mi355x_sd_abi_version() == 26
    assert hasattr(_lib.load(), "mi355x_sd_view_input") and hasattr(_lib.load(), "mi355x_sd_view_merge")


VALID = dict(scale=1.0, groups=2, batch=1, C=2, H=8, W=20, win_h=8, win_w=8, stride=4, ny=1, nx=4, circular=0, first=0, count=4)
N = 4096


def refused_calls(entry, base):
    """{what: (arguments by name, the word the message must hold)} of every call that must be refused, each one deviation from a
    valid call that is itself never made; the spans lie a spare block apart in a host buffer at `base`"""
    ok = dict(VALID, **{k: base + 4 * N * (2 * j) for j, k in enumerate(entry.spans)})
    src, dst = list(entry.spans)
    calls = {f"null {k}": (dict(ok, **{k: None}), k) for k in entry.spans}
    calls.update({f"{k} 0": (dict(ok, **{k: 0}), k) for k in entry.positive})
    calls.update({
        "window higher than the source": (dict(ok, win_h=9), "win_h"), "window wider than the source": (dict(ok, win_w=21, nx=1), "win_w"),
        "rows leave the source": (dict(ok, ny=2), "ny"), "columns leave the source": (dict(ok, nx=5), "nx"),
        "circular, narrower than the window": (dict(ok, circular=1, W=7, nx=1), "win_w"),
        "circular, a view starts past the source": (dict(ok, circular=1, nx=6), "nx"),
        "source past int64": (dict(ok, H=2 ** 31 - 1, W=2 ** 31 - 1, batch=2 ** 10, C=2 ** 10), "past int64_t"),
        "out on the last element of the source": (dict(ok, **{dst: ok[src] + 4 * (entry.spans[src](ok) - 1)}), "overlap"),
        "source on the last element of out": (dict(ok, **{src: ok[dst] + 4 * (entry.spans[dst](ok) - 1)}), "overlap")})
    if entry.entry == "view_input":
        calls.update({"groups 0": (dict(ok, groups=0), "groups"), "groups 3": (dict(ok, groups=3), "groups"),
                      "first -1": (dict(ok, first=-1), "first"), "count -1": (dict(ok, count=-1), "count"),
                      "first + count past the views": (dict(ok, first=2, count=3), "first")})
    unsupported = {"planes past the grid": dict(ok, C=65536, W=8, nx=1, count=1, groups=1)}
    return ok, calls, unsupported


@pytest.mark.parametrize("entry", list(ENTRIES.values()), ids=list(ENTRIES))
def test_the_description_refuses_what_it_says(entry):
    ok, calls, unsupported = refused_calls(entry, 1 << 20)
    assert refused(entry, ok) is None and refused(entry, dict(ok, circular=1, nx=5)) is None
    for what, (a, _) in calls.items():
        assert refused(entry, a) not in (None, "unsupported"), what
    for what, a in unsupported.items():
        far = {k: (j + 1) << 44 for j, k in enumerate(entry.spans)}
        assert refused(entry, dict(a, **far)) == "unsupported", what


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses: with a device a call that is not refused would launch on them")
@pytest.mark.parametrize("entry", list(ENTRIES.values()), ids=list(ENTRIES))
def test_every_refusal_is_refused_before_the_device_and_names_the_argument(entry):
    lib = _lib.load()
    buf = torch.full((8 * N,), 7.25)
    _, calls, unsupported = refused_calls(entry, buf.data_ptr())
    fn = getattr(lib, "mi355x_sd_" + entry.entry)
    for what, (a, word) in calls.items():
        assert fn(*[a.get(n) for _, n in entry.params]) == 1, what                                # MI355X_SD_ERR_INVALID
        msg = lib.mi355x_sd_last_error().decode()
        assert msg.startswith(f"mi355x_sd_{entry.entry}:") and word in msg, (what, msg)
    plane = 65536 * 8 * 8                                     # both spans of the well-formed, unsupported call
    big = torch.full((2 * plane + 64,), 7.25)
    for what, a in unsupported.items():
        assert all(f(a) == plane for f in entry.spans.values())
        a = dict(a, **{k: big.data_ptr() + 4 * j * (plane + 32) for j, k in enumerate(entry.spans)})
        assert fn(*[a.get(n) for _, n in entry.params]) == 2, what                                # MI355X_SD_ERR_UNSUPPORTED
    assert bool((buf == 7.25).all()) and bool((big == 7.25).all())
