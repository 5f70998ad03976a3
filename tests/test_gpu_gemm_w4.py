"""-m gpu: the four-wave GEMM tile (csrc/gemm_w4.hip) against a kernel that really is different, and against float64 math.

Reference: the generic double-buffered loop of csrc/gemm.hip on the 256 x 256 tile (MI355X_SD_GEMM_TILE=256 with MI355X_SD_NO_PIPE,
MI355X_SD_GEMM_NO_BIAS_ACC, MI355X_SD_NO_SPLITK, MI355X_SD_NO_W4): the same v_mfma_f32_16x16x32 products in the same K order, the
bias added after the sum, the epilogue operands in the same order -> the same bits (the WS cases excepted: WS_NOTE). New side: the four-wave tile forced at 256 x 256
(id 258) and 256 x 160 (id 259), and the picker's own choice. Every case of tests/gemm_w4_child.py is also held to the elementwise
float64 bound of tests/gemm_bounds.py over its whole output (both sides), and its MI355X_SD_GEMM_LOG route proves it reached the
kernel it is named for (four-wave on the new side, the generic 256 x 256 loop on the reference side)."""
import math

import pytest
import torch

from tests import gemm_bounds as GB
from tests.gemm_w4_child import CASES
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
REF = {"MI355X_SD_GEMM_TILE": "256", "MI355X_SD_NO_PIPE": "1", "MI355X_SD_GEMM_NO_BIAS_ACC": "1", "MI355X_SD_NO_SPLITK": "1",
       "MI355X_SD_NO_W4": "1"}
REL_BAR = 4e-3   # rel-L2 bar of the GEMM variant cases (tests/test_gpu_gemm_variants.py), bf16 stores


CHILD = Family("gemm_w4_child.py", "W4_JSON", "MI355X_SD_GEMM_LOG", timeout=600)


def _run(env_extra, names=(), dbg=True):
    return CHILD.child(names, env_extra, dbg)


def _family(name, bn):
    kind = CASES[name][3]
    ex = kind.startswith(("gate+R", "ws-gate+R")) or kind in ("R", "c-remap", "a-remap")
    return f"w4/{bn}" + ("+ex" if ex else "") + ("+ws" if kind.startswith("ws") else "")


# WS_NOTE. The widened-e4m3 (WS) cases hold the bound on both sides but are NOT bit-identical to the generic loop: the four-wave
# epilogue's `acc *= scale; acc + bias` sits in one basic block and -ffp-contract=fast makes it ONE fused multiply-add (the WS
# instantiations of gemm_w4_kernel carry 128 more v_pk_fma_f32 and 128 fewer v_pk_add_f32 than the 16-bit ones), while
# gemm_epilogue.h epi4 multiplies by the scale and adds the bias under a run-time `if (p.bias ...)`: two roundings. Same order, one
# fp32 rounding apart. Those cases compare the 256 x 160 form with the 256 x 256 form (same epilogue code, other tile) bit for bit.
def _is_ws(name):
    return CASES[name][3].startswith("ws")


def _route(v):
    assert len(v["route"]) == 1, v["route"]   # one launch per case
    return v["route"][0].split()[-1]


def _check_case(name, v, what):
    print(f"{what:>9} {name:<36} err/bound {v['ratio']:.3f}  rel {v['rel']:.2e}  {v['route']}")
    assert v["ratio"] < 1.0, (what, name, v)
    assert v["rel"] < REL_BAR, (what, name, v)
    assert v["guard"] in (None, 0), (what, name, v)   # canary rows / columns untouched


@pytest.mark.parametrize("tile,bn", [("258", 256), ("259", 160)], ids=["256x256", "256x160"])
def test_four_wave_tile_is_bit_identical_to_the_generic_loop(tile, bn):
    """Every case of the matrix (K = 192 .. 6144, one to several rounds of persistent blocks, ragged M / N, every epilogue, EX,
    WS, strided operands in guard bands) on the forced four-wave tile: inside the float64 bound, and the same bits as the generic
    loop. (GEGLU pairs sub-tiles: the 256 x 160 form has an odd number per wave and the launcher refuses it.)"""
    names = [n for n in CASES if bn == 256 or CASES[n][3] != "geglu"]
    ref, new = _run(REF, list(CASES)), _run({"MI355X_SD_GEMM_TILE": tile}, names)
    w256 = _run({"MI355X_SD_GEMM_TILE": "258"}, list(CASES))
    for k in names:
        _check_case(k, ref[k], "generic")
        _check_case(k, new[k], f"w4/{bn}")
        assert _route(ref[k]) == "generic/256", (k, ref[k]["route"])
        assert _route(new[k]) == _family(k, bn), (k, new[k]["route"])
        if _is_ws(k):   # (scale and bias in one FMA: see WS_NOTE) -- the two four-wave widths agree with each other instead
            assert new[k]["sha"] == w256[k]["sha"], (k, new[k], w256[k])
        else:
            assert new[k]["sha"] == ref[k]["sha"], (k, new[k], ref[k])


def test_picker_takes_the_four_wave_tile_and_matches_the_generic_loop():
    """The picker without a forced tile: every case flagged as a picker shape runs the four-wave 256 x 256 tile (fused QKV, FF1
    GEGLU, the MMDiT EX / WS forms, exactly 192 tiles) and gives the generic loop's bits; 186 tiles stay below its threshold."""
    names = [n for n in CASES if CASES[n][4]] + ["186 tiles (below the picker)"]
    ref, new = _run(REF, list(CASES)), _run({}, names)
    for k in names:
        _check_case(k, new[k], "picker")
        if CASES[k][4]:
            assert _route(new[k]) == _family(k, 256), (k, new[k]["route"])
            assert new[k]["sha"] == ref[k]["sha"] or _is_ws(k), (k, new[k], ref[k])   # (WS: WS_NOTE; held to the bound above)
        else:
            assert not _route(new[k]).startswith("w4"), (k, new[k]["route"])


def test_prologue_behind_the_stores_is_bit_identical_to_the_carried_prologue():
    """MI355X_SD_W4_SCHED=1: the next tile's prologue DMA goes out after the stores instead of ahead of them. Placement only: the
    same bits on the plain (non-EX, non-WS) 256 x 256 cases."""
    names = [n for n in CASES if not CASES[n][3].startswith(("gate+R", "ws")) and CASES[n][3] not in ("R", "c-remap", "a-remap")]
    base = _run({"MI355X_SD_GEMM_TILE": "258"}, list(CASES))
    got = _run({"MI355X_SD_GEMM_TILE": "258", "MI355X_SD_W4_SCHED": "1"}, names)
    for k in names:
        _check_case(k, got[k], "sched=1")
        assert _route(got[k]) == "w4/256", (k, got[k]["route"])
        assert got[k]["sha"] == base[k]["sha"], (k, got[k], base[k])


def test_fp16_build_four_wave_shapes_meet_the_fp64_bound():
    """The IEEE-half build (f16 MFMAs of the four-wave tile) on the picker-shaped cases: the float64 bound at u_out = 2^-10 over
    the whole output. (No route log in the production library: the debug build shares the picker code, and the test above proves
    these shapes reach the tile.)"""
    names = [n for n in CASES if CASES[n][4]]
    got = _run({"MI355X_SD_DTYPE": "fp16"}, names, dbg=False)
    for k in names:
        v = got[k]
        print(f"fp16 {k:<36} err/bound {v['ratio']:.3f}  rel {v['rel']:.2e}")
        assert v["ratio"] < 1.0, (k, v)
        assert v["rel"] < 6e-4, (k, v)   # (fp16 bar of tests/test_gpu_fp16.py: fp32 accumulation, one fp16 rounding)
        assert v["guard"] in (None, 0), (k, v)


def test_four_wave_race_screen():
    """The picker's four-wave shapes in the production library, 40 repetitions each with other-size GEMM launches interleaved every
    few repetitions (cache and DMA timing vary): every repetition bit-identical to the first, the first inside the float64 bound.
    Fused QKV, FF1 GEGLU, one EX gate + residual at K = 6144, one WS launch."""
    from paddlemix_amd import _lib, ops
    from paddlemix_amd.sd3 import dequantize_fp8_rows, quantize_fp8_rows
    ops.init(0)
    ed = _lib.elem_dtype()
    g = torch.Generator(device="cuda").manual_seed(77)
    noise_a = torch.randn(3000, 2048, device="cuda", generator=g).to(ed)
    noise_w = (torch.randn(1288, 2048, device="cuda", generator=g) / 45).to(ed)

    def operands(M, N, K):
        a = torch.randn(M, K, device="cuda", generator=g).to(ed)
        w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).to(ed)
        return a, w, torch.randn(N, device="cuda", generator=g)

    a, w, b = operands(8192, 3840, 1280)
    qkv = (lambda: ops.linear(a, w, b), (a, w), dict(bias=b))
    a2, w2, b2 = operands(8192, 10240, 1280)
    ff1 = (lambda: ops.linear(a2, w2, b2, geglu=True), (a2, w2), dict(bias=b2, geglu=True))
    a3, w3, b3 = operands(16384, 1536, 6144)
    gt = torch.randn(4, 1536, device="cuda", generator=g)
    r3 = torch.randn(16384, 1536, device="cuda", generator=g).to(ed)
    ex = (lambda: ops.linear_ex(a3, w3, b3, gate=gt, rows_per_batch=4096, residual=r3), (a3, w3),
          dict(bias=b3, gate=gt, rows_per_batch=4096, residual=r3))
    a4, _, b4 = operands(8192, 4608, 1536)
    w8, s8 = quantize_fp8_rows(torch.randn(4608, 1536, device="cuda", generator=g) / math.sqrt(1536))
    wsl = (lambda: ops.linear_ex(a4, w8, b4, w_scale=s8, gelu_tanh=True), (a4, dequantize_fp8_rows(w8, s8)), dict(bias=b4, act="gelu_tanh"))
    for name, (f, (aa, ww), kw) in {"qkv": qkv, "ff1 geglu": ff1, "ex gate+R": ex, "ws gelu": wsl}.items():
        first = f().clone()
        for i in range(40):
            if i % 4 == 0:
                ops.linear(noise_a, noise_w)
            assert torch.equal(f(), first), (name, i)
        ratio, rel = GB.bound_check(first, aa, ww, **kw)
        print(f"race screen {name}: err/bound {ratio:.3f} rel {rel:.2e}")
        assert ratio < 1.0 and rel < REL_BAR, (name, ratio, rel)
