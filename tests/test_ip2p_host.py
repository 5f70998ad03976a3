"""CPU tests of InstructPix2Pix (ABI 24): the loop of StableDiffusionDenoiser(image_guidance_scale=...) on the emulated device
(tests/abi_emulator_ip2p.py) against the line-by-line restatement of the reference's loop (tests/ip2p_ref.py), the host rules, and
the two entries' declarations, binding and refusals against one description of their operands (paddlemix_amd/ip2p_forms.py).

What "equal" means where:
  * without the rescale the product never enters x0 space, so it differs from the restatement by roundings. Per step, on identical
    inputs, the guided output is held to the bound of tests/ip2p_bounds.py against the float64 value of the reference's own lines
    (x0 conversions included; their float64 roundings are covered by a 1e-12 relative slack). The whole loop then ends within
    rtol = atol = 2e-5 of the float32 restatement on the same model outputs -- the tolerance tests/test_fused_vpred.py uses for a
    fused loop against the generic one.
  * with the rescale, the restatement with the emulator's arithmetic between the U-Net and ``scheduler.step`` (guide=), fed by the
    same emulated U-Net, must equal the fused_update=False loop bit for bit: the sigma index, the operand order, the triple order and
    the scaled input are all host logic. The fused loop differs from it by its tail's coefficient form only: 2e-5 again."""
import os
import re
from ctypes import c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from paddlemix_amd import _lib, ip2p_forms, ops
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import ip2p_bounds as IB
from tests import ip2p_cases as C
from tests import ip2p_ref as R
from tests.abi_emulator import Emulator, on_emulator
from tests.abi_emulator_ip2p import INT64_MAX, Ip2pEmulator, guidance3_math, refused
from tests.bound_pieces import check
from tests.header_decls import declared
from tests.step_pieces import Recording, Replay

CFG = C.UNETS["tiny8"]
P = synth_unet_params(CFG, seed=1234)


def _pipe(sched, emu=None, cfg=CFG, params=None):
    emu = emu or Ip2pEmulator()
    unet = Recording(on_emulator(UNet2DConditionModel, cfg, params or P, backend=emu))
    return StableDiffusionDenoiser(unet, C.SCHEDULERS[sched]()), emu, unet


def _call(pipe, inp, **kw):
    pe, ne, il, lat, added, neg = inp
    kw = dict(dict(num_inference_steps=C.STEPS, guidance_scale=C.GS, image_guidance_scale=C.GI, latents=lat.clone(), image=il,
                   added_cond_kwargs=added, negative_added_cond_kwargs=neg, generator=torch.Generator().manual_seed(7)), **kw)
    return pipe(pe, ne, **kw)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("sched", ["euler", "euler_a", "ddim", "dpm"])
def test_loop_without_rescale_against_the_restatement(sched, fused):
    inp = C.loop_inputs(CFG)
    pipe, emu, unet = _pipe(sched)
    before = []
    got = _call(pipe, inp, fused_update=fused, callback_on_step_end=lambda p, i, t, kw: (before.append(kw["latents"].clone()), kw)[1])
    assert emu.calls.count("ip2p_input") == emu.calls.count("guidance3") == len(unet.outs) == C.STEPS
    assert all(c["x"] is None and c["gr"] == 0.0 for c in emu.guidance3_calls)     # the flat form takes neither x nor coef
    sch = C.SCHEDULERS[sched]()
    seen = []
    want = R.loop(Replay(unet.config, unet.outs, dtype=torch.float32), sch, *inp[:4], C.STEPS, C.GS, C.GI, added=inp[4], negative_added=inp[5],
                  generator=torch.Generator().manual_seed(7), on_step=lambda *a: seen.append(a))
    xs = [inp[3] * float(sch.init_noise_sigma)] + before
    worst = 0.0
    for i, call in enumerate(emu.guidance3_calls):   # per step, on identical inputs: the latents and the U-Net output the product saw
        eps, x = call["eps"], xs[i].flatten(1)
        ref, e = IB.guidance3(eps, C.GS, C.GI)
        sigma = seen[i][5]
        if sigma is not None:                        # the reference's own lines in float64 (SD :391-409)
            s, xd = float(sigma), x.double()
            pt, pi, pu = (xd - s * v.double() for v in eps)
            ref64 = ((pu + C.GS * (pt - pi) + C.GI * (pi - pu)) - xd) / (-s)
            slack = 1e-12 * (xd.abs() / s + ref.abs())
            assert ((ref64 - ref).abs() <= slack + 1e-12).all()   # the conversion cancels: the weights sum to 1
            ref, e = ref64, e + slack
        ratio, _ = check(call["out"], ref, e, f32_rel=0.0)
        worst = max(worst, ratio)
    print(f"{sched} fused={fused}: worst |guided - float64 reference| / bound {worst:.3f}; |loop - restatement| "
          f"{float((got - want).abs().max()):.2e}")
    assert worst < 1.0
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("sched", ["euler", "euler_a", "ddim", "dpm"])
def test_loop_with_rescale_equals_the_restatement_with_the_emulators_arithmetic(sched):
    inp = C.loop_inputs(CFG)
    pipe, emu, unet = _pipe(sched)
    got = _call(pipe, inp, fused_update=False, guidance_rescale=C.GR)
    x0 = sched in C.SIGMA_SPACE
    assert all((c["x"] is not None) == x0 and c["gr"] == C.GR for c in emu.guidance3_calls)

    def guide(raw, latents, sigma):   # the product's rule: predicted originals only where the scheduler has sigmas
        B = latents.shape[0]
        res = guidance3_math(raw.reshape(3, B, -1), C.GS, C.GI, C.GR, latents.flatten(1) if x0 else None, sigma)
        return res.reshape(latents.shape)
    ref_unet = on_emulator(UNet2DConditionModel, CFG, P, backend=Emulator())
    want = R.loop(ref_unet, C.SCHEDULERS[sched](), *inp[:4], C.STEPS, C.GS, C.GI, C.GR, added=inp[4], negative_added=inp[5],
                  generator=torch.Generator().manual_seed(7), guide=guide)
    assert torch.equal(got, want)
    # the fused tail behind the same guidance: its coefficient form only
    pipe2, emu2, _ = _pipe(sched)
    fused = _call(pipe2, inp, guidance_rescale=C.GR)
    assert emu2.calls.count("guidance3") == C.STEPS
    assert torch.allclose(fused, got, rtol=2e-5, atol=2e-5)
    # and the reference's own rescale (torch.std, its order of operations) is what the emulator's statistics restate
    plain = R.loop(Replay(unet.config, unet.outs, dtype=torch.float32), C.SCHEDULERS[sched](), *inp[:4], C.STEPS, C.GS, C.GI, C.GR,
                   added=inp[4], negative_added=inp[5], generator=torch.Generator().manual_seed(7))
    assert torch.allclose(got, plain, rtol=2e-4, atol=2e-4), float((got - plain).abs().max())


def test_sdxl_shaped_loop_and_conditioning_order():
    cfg = C.UNETS["mini-xl8"]
    inp = C.loop_inputs(cfg)
    seen = []

    class Spy(Recording):
        def __call__(self, x, t, **kw):
            seen.append((x.clone(), kw["encoder_hidden_states"], kw["added_cond_kwargs"]))
            return super().__call__(x, t, **kw)
    emu = Ip2pEmulator()
    unet = Spy(on_emulator(UNet2DConditionModel, cfg, synth_unet_params(cfg, seed=5), backend=emu))
    pipe = StableDiffusionDenoiser(unet, C.SCHEDULERS["euler_a"]())
    got = _call(pipe, inp, num_inference_steps=2)
    pe, ne, il, lat, added, neg = inp
    x, enc, akw = seen[0]
    assert torch.equal(enc, torch.cat([pe, ne, ne]))                                               # [text, negative, negative]
    assert torch.equal(akw["text_embeds"], torch.cat([added["text_embeds"], neg["text_embeds"], neg["text_embeds"]]))
    assert torch.equal(akw["time_ids"], torch.cat([added["time_ids"]] * 3))
    assert torch.equal(x[:, 4:], torch.cat([il, il, torch.zeros_like(il)]))                        # [img, img, 0]
    assert torch.equal(x[:2, :4], x[2:4, :4]) and torch.equal(x[:2, :4], x[4:, :4]) and got.shape == lat.shape
    want = R.loop(Replay(unet.config, unet.outs, dtype=torch.float32), C.SCHEDULERS["euler_a"](), pe, ne, il, lat, 2, C.GS, C.GI,
                  added=added, negative_added=neg, generator=torch.Generator().manual_seed(7))
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-5)


def test_do_cfg_rule_and_image_latents():
    inp = C.loop_inputs(CFG)
    for gi, groups in ((0.99, 1), (1.0, 3)):                                                       # SD :764
        pipe, emu, _ = _pipe("ddim")
        _call(pipe, inp, image_guidance_scale=gi, num_inference_steps=1)
        assert emu.ip2p_input_calls[0]["groups"] == groups and emu.calls.count("guidance3") == (groups == 3)
    pipe, emu, _ = _pipe("ddim")
    _call(pipe, inp, guidance_scale=1.0, num_inference_steps=1)
    assert emu.ip2p_input_calls[0]["groups"] == 1 and "guidance3" not in emu.calls
    il = inp[2]
    with pytest.warns(FutureWarning, match=r"You have passed 2 text prompts \(`prompt`\), but only 1 initial images \(`image`\)\. Initial images "
                                           r"are now duplicating to match the number of text prompts\."):      # SD :724-731
        trip = pipe.prepare_ip2p_image_latents(il[:1], 2, True)
    assert torch.equal(trip, torch.cat([il[:1]] * 4 + [torch.zeros_like(il[:1])] * 2))
    assert torch.equal(pipe.prepare_ip2p_image_latents(il, 2, False), il)
    with pytest.raises(ValueError, match=r"Cannot duplicate `image` of batch size 2 to 3 text prompts\."):
        pipe.prepare_ip2p_image_latents(il, 3, True)
    with pytest.raises(ValueError, match="`image` has to be of type"):
        pipe.prepare_ip2p_image_latents([il], 2, True)
    with pytest.raises(ValueError, match="an image input needs a `vae`"):                          # pixels, and no VAE to encode them
        pipe.prepare_ip2p_image_latents(torch.zeros(2, 3, 64, 64), 2, True)


def test_channel_count_error_and_the_four_refusals():
    inp = C.loop_inputs(CFG)
    pe, ne, il, lat = inp[:4]
    four = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, C.configs.TINY, synth_unet_params(C.configs.TINY, seed=1),
                                               backend=Ip2pEmulator()), C.SCHEDULERS["ddim"]())
    with pytest.raises(ValueError, match=r"expects 4 but received `num_channels_latents`: 4 \+ `num_channels_image`: 4  = 8\. Please verify "
                                         r"the config of `pipeline.unet` or your `image` input\."):
        four(pe, ne, image=il, image_guidance_scale=1.5, latents=lat, num_inference_steps=1)
    pipe, _, _ = _pipe("ddim")
    kw = dict(image=il, image_guidance_scale=1.5, latents=lat, num_inference_steps=1)
    for name in ("mask_image", "control_image", "adapter_image"):
        with pytest.raises(NotImplementedError, match=f"`{name}` together with `image_guidance_scale`"):
            pipe(pe, ne, **kw, **{name: torch.zeros(2, 1, 8, 8)})
    lcm = dict(CFG, time_cond_proj_dim=32)
    distilled = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, lcm, synth_unet_params(lcm, seed=1), backend=Ip2pEmulator()),
                                        C.SCHEDULERS["ddim"]())
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        distilled(pe, ne, **kw)
    with pytest.raises(ValueError, match=r"`image` input cannot be undefined\."):
        pipe(pe, ne, image_guidance_scale=1.5, latents=lat, num_inference_steps=1)


def test_first_match_sigma_index_on_heun():
    """Heun repeats every timestep but the first: the reference's ``(timesteps == t).nonzero()[0]`` is the FIRST match, which on the
    second evaluation of a pair is not the scheduler's own step index"""
    inp = C.loop_inputs(CFG)
    for fused in (True, False):
        pipe, emu, _ = _pipe("heun")
        _call(pipe, inp, guidance_rescale=C.GR, num_inference_steps=3, fused_update=fused)
        sch = pipe.scheduler
        ts, sig = np.asarray(sch.timesteps), np.asarray(sch.sigmas, dtype=np.float32)
        assert len(ts) == 5 and ts[1] == ts[2] and sig[1] == sig[2] != sig[0]
        want = [float(sig[int(np.nonzero(ts == t)[0][0])]) for t in ts]
        assert [c["sigma"] for c in emu.guidance3_calls] == want
        rows = [c["coef"] for c in emu.guidance3_calls]
        assert rows[2] == rows[1] and rows[4] == rows[3] and rows[1] - rows[0] == 4 and rows[3] - rows[1] == 8   # one table, row pointers


def test_text2img_launch_list_is_unchanged_without_image_guidance_scale():
    """image_guidance_scale=None: a recorded text2img call issues the launches it issued before, and the same bits, before and after
    an InstructPix2Pix call on the same pipeline"""
    cfg4 = C.configs.TINY
    pe, ne, il, lat = C.loop_inputs(CFG)[:4]

    def text2img(pipe, emu):
        emu.calls.clear()
        out = pipe(pe, ne, num_inference_steps=2, guidance_scale=C.GS, latents=lat.clone(), generator=torch.Generator().manual_seed(3))
        return out, list(emu.calls)
    emu = Ip2pEmulator()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, cfg4, synth_unet_params(cfg4, seed=1), backend=emu), C.SCHEDULERS["euler_a"]())
    a, calls_a = text2img(pipe, emu)
    assert "ip2p_input" not in calls_a and "guidance3" not in calls_a and calls_a.count("ancestral_update") == 2
    pipe8, _, _ = _pipe("euler_a", emu)
    _call(pipe8, C.loop_inputs(CFG))
    b, calls_b = text2img(pipe, emu)
    assert calls_a == calls_b and torch.equal(a, b)


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_restatement_and_product_against_the_references_own_pipelines(name):
    """tests/golden/ip2p/loops.npz (scripts/make_ip2p_golden.py): the end latents of the reference's unmodified SD and SDXL
    InstructPix2Pix pipelines with its own schedulers around the closed-form stand-in U-Net, 4 steps. The restatement, in float32 with
    schedulers.py's classes, and the product loop on the emulator (fused and not) end there. 1e-4 of the largest latent: both sides are
    float32 loops of a few dozen operations per element that differ in the order of their roundings (the fused tails, the flat
    combine, numpy against tensor scalars), each worth a few 2^-24 of the operands, which reach the largest latent's size."""
    kind, sched, gr = C.GOLDEN[name]
    gold = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ip2p", "loops.npz"))[name])
    cfg = C.UNETS["tiny8" if kind == "sd" else "mini-xl8"]
    inp = C.loop_inputs(cfg, seed=C.GOLDEN_SEED)
    formula = C.FormulaUNet(_config(cfg))
    want = R.loop(formula, C.SCHEDULERS[sched](), *inp[:4], C.STEPS, C.GS, C.GI, gr, added=inp[4], negative_added=inp[5],
                  generator=torch.Generator().manual_seed(7))
    tol = 1e-4 * float(gold.abs().max())
    print(f"{name}: |restatement - reference| {float((want - gold).abs().max()):.2e} of {float(gold.abs().max()):.1f}")
    assert float((want - gold).abs().max()) < tol
    for fused in (True, False):
        emu = Ip2pEmulator()
        formula._lib, formula._emulated = emu, True
        got = _call(StableDiffusionDenoiser(formula, C.SCHEDULERS[sched]()), inp, guidance_rescale=gr, fused_update=fused)
        assert all((c["x"] is not None) == (gr > 0 and sched in C.SIGMA_SPACE) for c in emu.guidance3_calls), name
        assert float((got - gold).abs().max()) < tol, (name, fused, float((got - gold).abs().max()))


def _config(cfg):
    from types import SimpleNamespace
    return SimpleNamespace(**dict(dict(time_cond_proj_dim=None, sample_size=8), **cfg))


# ---------------------------------------------------------------------------------------------------- header, binding, refusals
CTYPES = {"const float*": c_void_p, "float*": c_void_p, "void*": c_void_p, "int": c_int, "float": c_float, "int64_t": c_int64}


@pytest.mark.parametrize("name", list(ip2p_forms.ENTRIES))
def test_entry_is_its_declaration_in_the_header(name):
    entry = ip2p_forms.ENTRIES[name]
    ret, params = declared()["mi355x_sd_" + entry.entry]
    assert ret == "int" and params == [tuple(p) for p in entry.params]
    assert all((kind == "float*") == (n in entry.written) for kind, n in params if kind.endswith("float*"))
    restype, argtypes = _lib.SIGNATURES["mi355x_sd_" + entry.entry]
    assert restype is c_int and list(argtypes) == [CTYPES[kind] for kind, _ in params] and (restype, argtypes) == ip2p_forms.signature(entry)
    assert set(entry.spans) == {n for kind, n in params if kind.endswith("float*")} and set(entry.written) <= set(entry.spans)
    assert callable(getattr(ops, entry.entry))


def test_abi_version_24_in_header_binding_and_library():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_sd.h")).read()
    abi = int(re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION >= 24
    assert _lib.load().mi355x_sd_abi_version() == abi


N = 4096
VALID = {"guidance3": dict(guidance_scale=7.5, image_guidance_scale=1.5, guidance_rescale=0.7, batch=1, per_sample=N),
         "ip2p_input": dict(scale=0.5, groups=3, batch=1, c_lat=4, c_img=4, hw=N // 8)}


def refused_calls(entry, base):
    """{what: arguments by name} of every call the row says must be refused, each one deviation from a valid call that is itself never
    made: the spans one spare plane apart in a host buffer at `base`"""
    ok, slot = dict(VALID[entry.entry]), 0
    for k, f in entry.spans.items():
        ok[k] = base + 4 * N * slot
        slot += f(dict(ok, **{p: 0 for p in entry.spans})) // N + 2
    assert slot <= 16
    size = {k: f(ok) for k, f in entry.spans.items()}
    calls = {f"null {k}": dict(ok, **{k: None}) for k in entry.spans if k not in entry.optional}
    for w in entry.written:
        for r in entry.spans:
            if r != w:
                calls[f"{r} on the last element of {w}"] = dict(ok, **{r: ok[w] + 4 * (size[w] - 1)})
                calls[f"{w} on the last element of {r}"] = dict(ok, **{w: ok[r] + 4 * (size[r] - 1)})
    calls.update({f"{k} 0": dict(ok, **{k: 0}) for k in entry.positive})
    last = entry.positive[-1]
    calls["far past int64"] = dict(ok, **{last: 2 ** 62})
    calls["one element past int64"] = dict(ok, **{last: INT64_MAX // 4 // (max(size.values()) // ok[last]) + 1})
    if entry.entry == "guidance3":
        calls["per_sample 1 under the rescale"] = dict(ok, per_sample=1)
    return ok, calls


@pytest.mark.parametrize("name", list(ip2p_forms.ENTRIES))
def test_the_description_refuses_what_it_says(name):
    """the table itself (what the emulator asserts): every generated call is refused, the valid one and the calls that leave an unused
    operand null or overlapping are not"""
    entry = ip2p_forms.ENTRIES[name]
    ok, calls = refused_calls(entry, 1 << 20)
    assert refused(entry, ok) is None
    for what, a in calls.items():
        assert refused(entry, a) is not None, what
    if name == "guidance3":
        flat = dict(ok, guidance_rescale=0.0)
        assert refused(entry, dict(flat, x=None, coef=None)) is None and refused(entry, dict(flat, x=ok["out"], coef=ok["out"])) is None
        assert refused(entry, dict(ok, x=None, coef=None)) is None and refused(entry, dict(ok, per_sample=2)) is None
        assert refused(entry, dict(flat, per_sample=1)) is None
        assert refused(entry, dict(ok, coef=None)) == "null pointer (coef)"                    # x without coef


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses: with a device a call that is not refused would launch on them")
@pytest.mark.parametrize("name", list(ip2p_forms.ENTRIES))
def test_every_refusal_of_the_description_is_refused_before_the_device(name):
    entry, lib = ip2p_forms.ENTRIES[name], _lib.load()
    buf = torch.full((16 * N,), 7.25)
    assert buf.data_ptr() % 16 == 0
    _, calls = refused_calls(entry, buf.data_ptr())
    fn = getattr(lib, "mi355x_sd_" + entry.entry)
    for what, a in calls.items():
        assert fn(*[a.get(n) for _, n in entry.params]) == 1, (entry.entry, what)               # MI355X_SD_ERR_INVALID
        msg = lib.mi355x_sd_last_error().decode()
        assert msg.startswith(f"mi355x_sd_{entry.entry}:"), (what, msg)
        reason = refused(entry, a)
        assert reason == "range" or reason in msg, (what, reason, msg)                          # by name
    assert bool((buf == 7.25).all())
