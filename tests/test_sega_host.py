"""CPU tests of semantic guidance (ABI 25): the recorded loops of the reference's own pipeline against the restatement
(tests/sega_ref.py), the loop of StableDiffusionDenoiser(editing_prompt_embeds=...) on the emulated device
(tests/abi_emulator_sega.py) against the restatement, the per-step table against the reference's decisions, the host and entry
refusals, the unchanged text2img loop, and the emulator's selection against torch.quantile on the kernel matrix."""
import os
import re
from ctypes import c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from paddlemix_amd import _lib, ops
from paddlemix_amd import sega_forms as SF
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests import configs
from tests import sega_bounds as SB
from tests import sega_cases as C
from tests import sega_ref as R
from tests.abi_emulator import on_emulator
from tests.abi_emulator_sega import ENTRY, INT64_MAX, SegaEmulator, parse_row, refused, sega_math
from tests.header_decls import declared
from tests.step_pieces import Recording, Replay

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sega", "loops.npz"))
# The loop tolerance, as tests/test_ip2p_host.py sets its own: both sides are float32 loops of a few dozen operations per element
# and step that differ in the order of their roundings -- numpy-scalar against tensor-scalar schedule coefficients, the fused tails'
# coefficient form, fma against separate products in the concept sums -- each worth a few 2^-24 of operands that reach the largest
# latent's size. 5 steps (Heun: 3) of at most ~50 such roundings: 2^10 * 2^-24 of the largest latent, stated before any run.
LOOP_TOL = 2.0 ** -14


def _config():
    from types import SimpleNamespace
    return SimpleNamespace(time_cond_proj_dim=None, addition_embed_type=None, sample_size=C.HW, in_channels=4)


def _edit_call(name):
    sched, n, use_sem, edit = C.GOLDEN[name]
    pe, ne, ee, lat, sem = C.loop_inputs(n)
    steps = C.GOLDEN_STEPS.get(name, C.STEPS)
    return sched, n, steps, pe, ne, ee, lat, (sem if use_sem else None), edit


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_restatement_against_the_references_own_pipeline(name):
    sched, n, steps, pe, ne, ee, lat, sem, edit = _edit_call(name)
    gold = torch.from_numpy(GOLD[name])
    want = R.loop(C.FormulaUNet(_config()), C.SCHEDULERS[sched](), pe, ne, ee.reshape(n * C.BATCH, C.TOKENS, C.DIM), lat, steps, C.GS,
                  sem_guidance=sem, **edit)
    tol = LOOP_TOL * float(gold.abs().max())
    print(f"{name}: |restatement - reference| {float((want - gold).abs().max()):.2e} of {float(gold.abs().max()):.1f} (tolerance {tol:.2e})")
    assert torch.isfinite(gold).all() and float((want - gold).abs().max()) < tol


@pytest.mark.parametrize("fused_update", [True, False])
@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_denoiser_loop_on_the_emulator_against_the_restatement_and_the_record(name, fused_update):
    sched, n, steps, pe, ne, ee, lat, sem, edit = _edit_call(name)
    formula, emu = C.FormulaUNet(_config()), SegaEmulator()
    formula._lib, formula._emulated = emu, True
    pipe = StableDiffusionDenoiser(formula, C.SCHEDULERS[sched]())
    kw = dict(num_inference_steps=steps, guidance_scale=C.GS, latents=lat.clone(), editing_prompt_embeds=ee, sem_guidance=sem,
              fused_update=fused_update, **edit)
    got = pipe(pe, ne, **kw)
    iters = len(pipe.scheduler.timesteps)
    assert emu.calls.count("sega_guidance") == iters and all((c["extra"] is not None) == (sem is not None) for c in emu.sega_calls)
    rows = [c["row_ptr"] for c in emu.sega_calls]
    assert [b - a for a, b in zip(rows, rows[1:])] == [4 * SF.row_words(n)] * (iters - 1)          # one table, row pointers
    want = R.loop(formula, C.SCHEDULERS[sched](), pe, ne, ee.reshape(n * C.BATCH, C.TOKENS, C.DIM), lat, steps, C.GS, sem_guidance=sem, **edit)
    torch_ops = pipe(pe, ne, **dict(kw, fused_guidance=False))
    assert emu.calls.count("sega_guidance") == iters                                               # (the torch-op path launches none)
    tol = LOOP_TOL * float(want.abs().max())
    gold = torch.from_numpy(GOLD[name])
    print(f"{name} fused_update={fused_update}: |loop - restatement| {float((got - want).abs().max()):.2e} |torch ops - restatement| "
          f"{float((torch_ops - want).abs().max()):.2e} |loop - record| {float((got - gold).abs().max()):.2e} (tolerance {tol:.2e})")
    assert float((got - want).abs().max()) < tol and float((torch_ops - want).abs().max()) < tol
    assert float((got - gold).abs().max()) < tol
    # [n, T, D] serves every sample: the same batch, concept-major
    same = pipe(pe, ne, **dict(kw, editing_prompt_embeds=ee[:, 0]))
    assert torch.equal(same, got)


def test_batch_order_is_negative_text_then_concept_major():
    pe, ne, ee, lat, _ = C.loop_inputs(2)
    ee = ee + torch.arange(2 * C.BATCH).reshape(2, C.BATCH, 1, 1)   # every (concept, sample) its own embedding
    seen = []

    class Spy(C.FormulaUNet):
        def __call__(self, x, t, encoder_hidden_states=None, **kw):
            seen.append((x.clone(), encoder_hidden_states))
            return super().__call__(x, t, encoder_hidden_states=encoder_hidden_states, **kw)
    spy = Spy(_config())
    spy._lib, spy._emulated = SegaEmulator(), True
    StableDiffusionDenoiser(spy, C.SCHEDULERS["ddim"]())(pe, ne, num_inference_steps=1, latents=lat.clone(), editing_prompt_embeds=ee)
    x, enc = seen[0]
    assert torch.equal(enc, torch.cat([ne, pe, ee[0], ee[1]])) and x.shape[0] == 4 * C.BATCH
    assert all(torch.equal(x[:C.BATCH], x[k * C.BATCH:(k + 1) * C.BATCH]) for k in range(4))


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_row_table_is_the_references_per_step_decisions(name):
    """every row against the reference's own lines (REF :581-613, :653-691) restated independently here, regime by regime"""
    sched, n, steps, _, _, _, _, _, edit = _edit_call(name)
    iters = 2 * steps - 1 if sched == "heun" else steps
    hw = C.HW * C.HW
    table = SF.rows(iters, n, hw, C.GS, edit.get("edit_momentum_scale", 0.1), edit.get("edit_mom_beta", 0.4),
                    **{k: v for k, v in edit.items() if k not in ("edit_momentum_scale", "edit_mom_beta")})
    assert table.shape == (iters, SF.row_words(n)) and table.dtype == np.uint32
    regimes = set()
    pick = lambda v, c: v[c] if isinstance(v, list) else v   # noqa: E731
    for i in range(iters):
        r = parse_row(table[i], n)
        warm, w = [], torch.zeros(n)
        for c in range(n):
            if i >= pick(edit.get("edit_warmup_steps", 10), c):
                warm.append(c)
            cd = edit.get("edit_cooldown_steps")
            cd = cd[c] if isinstance(cd, list) else (i + 1 if cd is None else cd)
            pc = r["per"][c]
            assert bool((r["active"] >> c) & 1) == (i < cd)
            if i >= cd:
                continue
            w[c] = edit["edit_weights"][c] if edit.get("edit_weights") else 1.0
            s = torch.tensor(float(pick(edit.get("edit_guidance_scale", 5), c)))
            assert float(pc["scale"]) == float(-s if pick(edit.get("reverse_editing_direction", False), c) else s)
            rank = torch.tensor(pick(edit.get("edit_threshold", 0.9), c), dtype=torch.float32) * (hw - 1)      # torch.quantile's rank
            assert pc["lo"] == int(rank.floor()) and float(pc["frac"]) == float(rank - rank.floor())
        assert r["warm"] == sum(1 << c for c in warm)
        assert r["regime"] == (2 if len(warm) == n else (1 if warm else 0))
        regimes.add(r["regime"])
        full = torch.nan_to_num(torch.where(w < 0, torch.zeros_like(w), w))
        assert [float(p["w_full"]) for p in r["per"]] == full.tolist()
        if r["regime"] == 1:
            cw = torch.where(w[warm] < 0, torch.zeros(len(warm)), w[warm])
            cw = cw / cw.sum(dim=0)
            np.testing.assert_array_equal(np.array([float(r["per"][c]["w_part"]) for c in warm], dtype=np.float32), cw.numpy())
        assert (float(r["gs"]), float(r["ms"]), float(r["beta"])) == tuple(float(np.float32(v)) for v in (
            C.GS, edit.get("edit_momentum_scale", 0.1), edit.get("edit_mom_beta", 0.4)))
        assert float(r["omb"]) == float(np.float32(1 - edit.get("edit_mom_beta", 0.4)))
    if n == 2 and isinstance(edit.get("edit_warmup_steps"), list):
        assert regimes == {1, 2}                                     # warm-ups [0, 2]: partial, then all
    if name == "euler_two_scalars":
        assert regimes == {0, 2}                                     # a scalar warm-up of 2: none, then all


def test_partial_regime_with_a_zero_weight_sum_is_nan_as_in_the_reference():
    table = SF.rows(1, 2, 64, C.GS, edit_warmup_steps=[0, 5], edit_weights=[-1.0, 1.0])
    r = parse_row(table[0], 2)
    assert r["regime"] == 1 and np.isnan(r["per"][0]["w_part"]) and float(r["per"][0]["w_full"]) == 0.0


def test_host_refusals_each_by_name():
    pe, ne, ee, lat, _ = C.loop_inputs(1)
    formula = C.FormulaUNet(_config())
    formula._lib, formula._emulated = SegaEmulator(), True
    pipe = StableDiffusionDenoiser(formula, C.SCHEDULERS["ddim"]())
    kw = dict(num_inference_steps=1, latents=lat.clone(), editing_prompt_embeds=ee)
    with pytest.raises(NotImplementedError, match="`guidance_scale` > 1"):
        pipe(pe, ne, guidance_scale=1.0, **kw)
    plane = torch.zeros(2, 1, 8, 8)
    for name, v in (("guidance_rescale", 0.7), ("image_guidance_scale", 1.5), ("image", plane), ("mask_image", plane),
                    ("control_image", plane), ("adapter_image", plane), ("added_cond_kwargs", {"text_embeds": plane})):
        with pytest.raises(NotImplementedError, match=f"`{name}` together with editing prompts"):
            pipe(pe, ne, **kw, **{name: v})
    xl = C.FormulaUNet(_config())
    xl.config.addition_embed_type = "text_time"
    xl._lib, xl._emulated = SegaEmulator(), True
    with pytest.raises(NotImplementedError, match="addition_embed_type"):
        StableDiffusionDenoiser(xl, C.SCHEDULERS["ddim"]())(pe, ne, **kw)
    lcm = C.FormulaUNet(_config())
    lcm.config.time_cond_proj_dim = 32
    lcm._lib, lcm._emulated = SegaEmulator(), True
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        StableDiffusionDenoiser(lcm, C.SCHEDULERS["ddim"]())(pe, ne, **kw)
    from paddlemix_amd.export import ExportedProgram
    prog = ExportedProgram.__new__(ExportedProgram)
    with pytest.raises(NotImplementedError, match="exported program"):
        StableDiffusionDenoiser(prog, C.SCHEDULERS["ddim"]())(pe, ne, **kw)
    with pytest.raises(NotImplementedError, match="1 .. 8 editing prompts"):
        pipe(pe, ne, **dict(kw, editing_prompt_embeds=ee.expand(9, -1, -1, -1)))
    with pytest.raises(ValueError, match="edit_threshold"):
        pipe(pe, ne, edit_threshold=1.5, **kw)
    with pytest.raises(ValueError, match="`sem_guidance`: expected at least 1 planes"):
        pipe(pe, ne, sem_guidance=torch.zeros(0, *lat.shape), **kw)
    with pytest.raises(ValueError, match="`editing_prompt_embeds`: expected"):
        pipe(pe, ne, **dict(kw, editing_prompt_embeds=ee[:, :1]))


def test_text2img_plan_and_calls_are_unchanged_without_editing_prompts():
    """no editing prompt: a text2img call issues the launches it issued before and the same bits, before and after a semantic-guidance
    call through the same library; the edit_* defaults alone change nothing"""
    cfg = configs.TINY
    lat = C.loop_inputs(1)[3]
    g = torch.Generator().manual_seed(5)
    pe, ne, ee = (torch.randn(*shape, C.TOKENS, cfg["cross_attention_dim"], generator=g) for shape in ((C.BATCH,), (C.BATCH,), (1, C.BATCH)))
    emu = SegaEmulator()
    unet = on_emulator(UNet2DConditionModel, cfg, synth_unet_params(cfg, seed=1), backend=emu)
    pipe = StableDiffusionDenoiser(unet, C.SCHEDULERS["euler"]())

    def text2img(**kw):
        emu.calls.clear()
        out = pipe(pe, ne, num_inference_steps=2, guidance_scale=C.GS, latents=lat.clone(), **kw)
        return out, list(emu.calls)
    a, calls_a = text2img()
    plans_a = len(unet._plans) if hasattr(unet, "_plans") else None
    assert "sega_guidance" not in calls_a
    emu.calls.clear()
    edited = pipe(pe, ne, num_inference_steps=2, guidance_scale=C.GS, latents=lat.clone(), editing_prompt_embeds=ee, edit_warmup_steps=0)
    assert emu.calls.count("sega_guidance") == 2
    assert not torch.equal(edited, a)
    b, calls_b = text2img(edit_guidance_scale=9, edit_threshold=0.5, sem_guidance=[lat, lat])
    assert calls_a == calls_b and torch.equal(a, b)
    if plans_a is not None:
        assert len(unet._plans) == plans_a + 1                       # the (2 + n) B batch is one more plan; the text2img plan is reused


# ---------------------------------------------------------------------------------------------------- the quantile rule
@pytest.mark.parametrize("name", [k for k, v in C.KERNEL.items() if v["hw"] <= 16384])
def test_emulators_select_is_torch_quantile_and_the_cases_have_no_element_near_a_threshold(name):
    """the emulator's v[lo], v[hi] are the sort's, its threshold is torch.quantile's bit for bit, NaN with NaN; and the reference
    has no |g| within an ulp of an inexact threshold on any kernel case, so the GPU test compares the whole mask"""
    spec = C.KERNEL[name]
    eps, mom, extra, row = C.kernel_inputs(spec, seed=sorted(C.KERNEL).index(name))
    n = spec["n"]
    out, mom2, stats = sega_math(eps, mom, extra, row.numpy(), n)
    ref = SB.reference(eps, mom, extra, row.numpy(), n, spec["q"])
    live = [c for c in range(n) if (parse_row(row.numpy(), n)["active"] >> c) & 1]
    assert ref["near"] == 0
    for c in live:
        assert torch.equal(stats[c, ..., 0].view(torch.int32), ref["vlo"][c].view(torch.int32))
        assert torch.equal(stats[c, ..., 1].view(torch.int32), ref["vhi"][c].view(torch.int32))
        thr, want = stats[c, ..., 2], ref["thr_ref"][c]
        assert torch.equal(torch.isnan(thr), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(thr).view(torch.int32), torch.nan_to_num(want).view(torch.int32)), (thr, want)
    assert SB.check_thr(stats[live, ..., 2], ref["vlo"][live], ref["vhi"][live], ref["thr64"][live]) == 0
    ro, bad_o = SB.check_values(out, ref["out"], ref["e_out"])
    rm, bad_m = SB.check_values(mom2, ref["mom"], ref["e_mom"])
    assert ro < 1.0 and rm < 1.0 and bad_o == 0 and bad_m == 0, (ro, rm, bad_o, bad_m)


# ---------------------------------------------------------------------------------------------------- header, binding, refusals
CTYPES = {"const float*": c_void_p, "float*": c_void_p, "void*": c_void_p, "int": c_int, "float": c_float, "int64_t": c_int64}


def test_entry_is_its_declaration_in_the_header():
    ret, params = declared()["mi355x_sd_" + ENTRY.entry]
    assert ret == "int" and params == [tuple(p) for p in ENTRY.params]
    assert all((kind == "float*") == (n in ENTRY.written) for kind, n in params if kind.endswith("float*"))
    restype, argtypes = _lib.SIGNATURES["mi355x_sd_" + ENTRY.entry]
    assert restype is c_int and list(argtypes) == [CTYPES[kind] for kind, _ in params]
    assert set(ENTRY.spans) == {n for kind, n in params if kind.endswith("float*")} and callable(ops.sega_guidance)


def test_abi_version_25_in_header_binding_and_library():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mi355x_sd.h")).read()
    abi = int(re.search(r"#define MI355X_SD_ABI_VERSION (\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION >= 25
    assert _lib.load().mi355x_sd_abi_version() == abi
    assert hasattr(_lib.load(), "mi355x_sd_sega_guidance")


N = 4096
VALID = dict(n_concepts=2, batch=1, channels=4, hw=N // 4)


def refused_calls(base):
    """{what: arguments by name} of every call the row says must be refused, each one deviation from a valid call that is itself
    never made: the spans at least one spare plane apart in a host buffer at `base`"""
    ok, slot = dict(VALID), 0
    for k, f in ENTRY.spans.items():
        ok[k] = base + 4 * N * slot
        slot += -(-f(dict(ok, **{p: 0 for p in ENTRY.spans})) // N) + 1
    assert slot <= 16
    size = {k: f(ok) for k, f in ENTRY.spans.items()}
    calls = {f"null {k}": dict(ok, **{k: None}) for k in ENTRY.spans if k not in ENTRY.optional}
    for w in ENTRY.written:
        for r in ENTRY.spans:
            if r != w:
                calls[f"{r} on the last element of {w}"] = dict(ok, **{r: ok[w] + 4 * (size[w] - 1)})
                calls[f"{w} on the last element of {r}"] = dict(ok, **{w: ok[r] + 4 * (size[r] - 1)})
    calls.update({f"{k} 0": dict(ok, **{k: 0}) for k in ENTRY.positive})
    calls["far past int64"] = dict(ok, hw=2 ** 62)
    calls["one element past int64"] = dict(ok, hw=INT64_MAX // 4 // (size["eps"] // ok["hw"]) + 1)
    unsupported = {"nine concepts": dict(ok, n_concepts=9), "a plane of 65537": dict(ok, hw=65537)}
    return ok, calls, unsupported


def test_the_description_refuses_what_it_says():
    ok, calls, unsupported = refused_calls(1 << 20)
    assert refused(ENTRY, ok) is None and refused(ENTRY, dict(ok, extra=None, stats=None)) is None
    for what, a in calls.items():
        assert refused(ENTRY, a) not in (None, "unsupported"), what
    for what, a in unsupported.items():
        far = {k: (j + 1) << 40 for j, k in enumerate(ENTRY.spans)}
        assert refused(ENTRY, dict(a, **far)) == "unsupported", what


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses: with a device a call that is not refused would launch on them")
def test_every_refusal_of_the_description_is_refused_before_the_device():
    lib = _lib.load()
    buf = torch.full((16 * N,), 7.25)
    assert buf.data_ptr() % 16 == 0
    _, calls, unsupported = refused_calls(buf.data_ptr())
    fn = lib.mi355x_sd_sega_guidance
    for what, a in calls.items():
        assert fn(*[a.get(n) for _, n in ENTRY.params]) == 1, what                                  # MI355X_SD_ERR_INVALID
        msg = lib.mi355x_sd_last_error().decode()
        assert msg.startswith("mi355x_sd_sega_guidance:"), (what, msg)
        reason = refused(ENTRY, a)
        assert reason == "range" or reason in msg, (what, reason, msg)                              # by name
    big = torch.full((2 * 4 * 65537 * 4 + 64,), 7.25)          # room for every span of the two well-formed, unsupported calls
    for what, a in unsupported.items():
        a = dict(a, eps=big.data_ptr(), momentum=buf.data_ptr(), out=buf.data_ptr() + 4 * 5 * N, row=buf.data_ptr() + 4 * 11 * N,
                 extra=None, stats=None)
        if a["hw"] > N:                                         # (momentum and out of 4 * 65537 floats do not fit the small buffer)
            continue
        assert fn(*[a.get(n) for _, n in ENTRY.params]) == 2, what                                  # MI355X_SD_ERR_UNSUPPORTED
    assert bool((buf == 7.25).all()) and bool((big == 7.25).all())
