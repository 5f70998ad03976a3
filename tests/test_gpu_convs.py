"""-m gpu: every convolution kernel form against float64 math on inputs that expose a wrong gather.

mi355x_sd_conv3x3 is an implicit GEMM whose A operand is gathered per lane from an NHWC image; the gather is written three times
(csrc/gemm.hip, gemm_pipe.hip, gemm256.hip) and instantiated per tile. The case matrix of tests/conv_cases.py -- coded input with
one-hot weights and padding masks (compared exactly), random data with every epilogue operand (held to the elementwise bound of
tests/conv_bounds.py), stride 1 / 2, upsample, both padding rules, both K orders, Cin = 8 .. 640, one pixel to 259 row tiles, x in a
NaN buffer, the output in a canary buffer -- runs under every forced tile family of the debug-switch build, with and without the
pipelined loops, with and without split-K, and under the picker; the MI355X_SD_GEMM_LOG route of every case must be the family the
run names or its tabled fallback. The three direct kernels of csrc/misc.hip have their own selectors and bounds."""
import pytest

from tests.conv_cases import CASES, GEOMS, out_hw
from tests.gpu_child import RUNNER, Family

pytestmark = pytest.mark.gpu
WS_BYTES = 32 << 20   # the split-K scratch ops.conv3x3 hands over (paddlemix_amd/ops.py _workspace)
# bias after the sum on both sides, as in tests/test_gpu_gemm_variants.py: then a tile's pipelined and generic loops give the same bits
FORCED_BASE = {"MI355X_SD_GEMM_NO_BIAS_ACC": "1"}


CHILD = Family("conv_child.py", "CONV_JSON", "MI355X_SD_GEMM_LOG", timeout=600)


def _spec(mode, env_extra, names=(), dbg=True):
    return CHILD.spec((mode, *names), env_extra, dbg)


def _all_runs():
    return ([("gemm", _forced_env(*r), (), True) for r in RUNS] + [("gemm", {"MI355X_SD_GEMM_TILE": str(t)}, BIAS_ACC_CASES, True) for t in PIPE_TILES]
            + [("gemm", {}, (), True), ("gemm", {"MI355X_SD_DTYPE": "fp16"}, (), False), ("direct", {}, (), False),
               ("direct", {"MI355X_SD_DTYPE": "fp16"}, (), False), ("wide", {}, (), True)])


def _run(mode, env_extra, names=(), dbg=True):
    """the child's JSON. The children of this file are independent processes (the switches are read once per process); the first call
    starts all of them, four at a time, each under its own time limit; after a child that died on the GPU none is started and the
    session ends (tests/gpu_child.py)."""
    RUNNER.run_many([_spec(*sp) for sp in _all_runs()], workers=4)
    return RUNNER.run(**_spec(mode, env_extra, names, dbg))


def _mnk(case):
    ho, wo = out_hw(case)
    return case.B * ho * wo, case.Cout, 9 * case.Cin


def _splitk(case):
    """csrc/gemm.hip plan_splitk on the 128 x 128 tile: at most 160 tiles, at least 8 K-tiles, slices of at least 4 K-tiles towards 416
    blocks, partial sums inside the workspace"""
    M, N, K = _mnk(case)
    tiles, nt = -(-M // 128) * -(-N // 128), -(-K // 64)
    if tiles > 160 or nt < 8:
        return False
    s = min(-(-416 // tiles), nt // 4, WS_BYTES // (M * N * 4))
    return s >= 2 and -(-nt // -(-nt // s)) >= 2


# FALLBACKS: where a launcher refuses a combination, the route the launch takes instead, with the line that refuses it.
#   pipe/<tile>  needs K % 64 == 0 (Cin = 8, 40: K = 72, 360)   gemm_pipe.hip launch_gemm_pipe: `if (off || (a.wscale && !a.w16) ||
#                (a.K & 63) || ...) return SD_ERR_UNSUPPORTED;` -> generic/<tile> (tile id 129 has no generic form: gemm.hip
#                dispatch_gemm's last line, generic/128)
#   gemm256      needs Cin % 64 == 0   gemm.hip dispatch_gemm: `if (tile == 257 && fits32 && !((a.K & 63) || (a.conv && (a.Cin & 63)) ||
#                a.a_rpb))` -> the next line, generic/256
#   kb64         needs Cin % 64 == 0   capi.hip mi355x_sd_conv3x3: "MI355X_SD_CONV_KB64 needs Cin % 64 == 0" -- an error, not a route:
#                no kb64 case has another Cin (tests/test_gpu_kernels.py test_conv3x3_kb64_weight_order checks the error)
#   +splitk      only the 128 x 128 tile is sliced   gemm.hip dispatch_gemm: `if (tile == 128) plan_splitk(a, 128, 128);`
def expected_route(tile, nopipe, nosplit, case):
    k64 = case.Cin % 64 == 0
    if tile == 257:
        return "gemm256" if k64 else "generic/256"
    if not nopipe and k64:
        fam = f"pipe/{tile}"
    else:
        fam = f"generic/{128 if tile == 129 else tile}"
    return fam + ("+splitk" if tile == 128 and not nosplit and _splitk(case) else "")


def _route(v):
    assert len(v["route"]) == 1, v["route"]   # one launch per case
    return v["route"][0].split()[-1]


def _check(name, v, what):
    assert v["mismatch"] in (None, 0), (what, name, v)   # selectors: exact
    assert v["ratio"] < 1.0, (what, name, v)             # random data: inside the float64 bound, every element
    assert v["guard"] in (None, 0), (what, name, v)      # canary rows / columns untouched


ATTRS = {"stride 1": lambda c: GEOMS[c.geom][0] == 1, "stride 2": lambda c: GEOMS[c.geom][0] == 2, "upsample": lambda c: GEOMS[c.geom][1],
         "pad_br": lambda c: GEOMS[c.geom][2], "kb64": lambda c: c.kb64, "plain K": lambda c: not c.kb64,
         "coded": lambda c: c.kind == "coded", "mask": lambda c: c.kind == "mask", "random": lambda c: c.kind == "random"}
FAMILIES = ["generic/128", "generic/160", "generic/256", "generic/320", "pipe/128", "pipe/129", "pipe/160", "pipe/256", "pipe/320",
            "gemm256", "generic/128+splitk", "pipe/128+splitk"]
PIPE_TILES = (128, 129, 160, 256, 320)
# the random cases with a bias whose K the pipelined loops take: run once more per tile WITHOUT MI355X_SD_GEMM_NO_BIAS_ACC, so that the
# production form of those loops (the bias is the accumulators' initial value, GemmArgs::bias_acc) is held to the bound on every tile
BIAS_ACC_CASES = tuple(n for n, c in CASES.items() if c.kind == "random" and "bias" in c.epi and c.Cin % 64 == 0)
RUNS = [(t, nopipe, False) for t in (128, 129, 160, 256, 257, 320) for nopipe in (False, True)] + [(128, False, True), (128, True, True)]


def _forced_env(tile, nopipe, nosplit):
    env = dict(FORCED_BASE, MI355X_SD_GEMM_TILE=str(tile))
    if nopipe:
        env["MI355X_SD_NO_PIPE"] = "1"
    if nosplit:
        env["MI355X_SD_NO_SPLITK"] = "1"
    return env


def _forced(tile, nopipe, nosplit):
    return _run("gemm", _forced_env(tile, nopipe, nosplit))


@pytest.mark.parametrize("tile,nopipe,nosplit", RUNS, ids=[f"tile{t}{'-nopipe' if p else ''}{'-nosplitk' if s else ''}" for t, p, s in RUNS])
def test_forced_family_runs_the_whole_matrix(tile, nopipe, nosplit):
    """every case on the forced tile: exact selectors, random data inside the bound, canaries untouched, and the logged route is the
    family this run names (or its tabled fallback)"""
    got = _forced(tile, nopipe, nosplit)
    worst = {}
    for name, case in CASES.items():
        v = got[name]
        _check(name, v, (tile, nopipe, nosplit))
        assert _route(v) == expected_route(tile, nopipe, nosplit, case), (name, v["route"], expected_route(tile, nopipe, nosplit, case))
        if case.kind == "random":
            worst[_route(v)] = max(worst.get(_route(v), 0.0), v["ratio"])
    print(f"tile {tile} nopipe {nopipe} nosplitk {nosplit}: worst err/bound per family {worst}")


def test_every_family_is_reached_by_every_flag_and_selector_kind():
    """the coverage condition, from the route logs of the forced runs: each family by stride 1, stride 2, upsample, pad_br, kb64, plain K
    order, and by both selector kinds"""
    seen, worst = {f: {a: 0 for a in ATTRS} for f in FAMILIES}, {f: 0.0 for f in FAMILIES}
    for run in RUNS:
        got = _forced(*run)
        for name, case in CASES.items():
            fam = _route(got[name])
            assert fam in seen, (run, name, fam)
            worst[fam] = max(worst[fam], got[name]["ratio"])
            for a, f in ATTRS.items():
                seen[fam][a] += bool(f(case))
    for fam in FAMILIES:
        print(f"{fam:<20} worst err/bound {worst[fam]:.3f}  cases " + "  ".join(f"{a} {n}" for a, n in seen[fam].items()))
    for fam in FAMILIES:
        for a in ATTRS:
            assert seen[fam][a] > 0, (fam, a)


@pytest.mark.parametrize("tile", [128, 129, 160, 256, 320])
def test_pipelined_and_generic_loops_of_one_tile_give_the_same_bits(tile):
    """within one K order the pipelined and the generic loop walk K identically (32-deep MFMA steps in K order, split-K slices summed
    in index order, bias after the sum on both sides): the same bits. (gemm256 and the other K order walk K differently: bound only.)"""
    a, b = _forced(tile, False, False), _forced(tile, True, False)
    n = 0
    for name, case in CASES.items():
        if _route(a[name]).startswith("pipe/"):
            assert _route(b[name]).startswith("generic/"), (name, b[name]["route"])
            assert a[name]["sha"] == b[name]["sha"], (tile, name, a[name], b[name])
            n += 1
    assert n > 20, n


@pytest.mark.parametrize("tile", PIPE_TILES)
def test_pipelined_loops_with_the_bias_in_the_accumulators(tile):
    """the forced runs above add the bias after the sum (so that two loops can be compared bit for bit); production starts the
    accumulators at the bias: every random case with a bias on each pipelined tile in that form, inside the bound"""
    got = _run("gemm", {"MI355X_SD_GEMM_TILE": str(tile)}, BIAS_ACC_CASES)
    assert len(BIAS_ACC_CASES) >= 10
    worst = 0.0
    for name in BIAS_ACC_CASES:
        _check(name, got[name], ("bias_acc", tile))
        assert _route(got[name]) == expected_route(tile, False, False, CASES[name]), (name, got[name]["route"])
        worst = max(worst, got[name]["ratio"])
    print(f"pipe/{tile} bias in the accumulators: worst err/bound {worst:.3f} over {len(BIAS_ACC_CASES)} cases")


def test_picker_routes_and_sdxl_shapes():
    """the picker without a forced tile: the whole matrix exact / inside the bound on some conv family; the VAE decoder's 512 -> 512
    conv at 128 x 128 reaches the phased 256 x 256 kernel and the UNet's 320 -> 320 conv a pipelined loop, both in the production K order"""
    got = _run("gemm", {})
    fams = {}
    for name in CASES:
        _check(name, got[name], "picker")
        fam = _route(got[name])
        assert fam in FAMILIES, (name, fam)
        fams.setdefault(fam, []).append(name)
        print(f"picker {name:<32} {fam:<20} err/bound {got[name]['ratio']:.3f}")
    assert _route(got["random sdxl vae 512 kb64"]) == "gemm256", got["random sdxl vae 512 kb64"]["route"]
    assert _route(got["random sdxl unet 320 kb64"]).startswith("pipe/"), got["random sdxl unet 320 kb64"]["route"]
    assert any(f.endswith("+splitk") for f in fams), fams.keys()


def test_fp16_build_whole_matrix():
    """the IEEE-half build (production library, no route log), picker: selectors exact, random cases inside the bound at u_out = 2^-10"""
    got = _run("gemm", {"MI355X_SD_DTYPE": "fp16"}, dbg=False)
    worst = 0.0
    for name in CASES:
        _check(name, got[name], "fp16")
        worst = max(worst, got[name]["ratio"])
    print(f"fp16 build: worst err/bound {worst:.3f} over {len(CASES)} cases")


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_direct_kernels(build):
    """conv_in3x3 (Cin = 4 unrolled and Cin = 8 rolled, with and without in_scale, 16-bit and fp32 output, W = 7), conv_out3x3 (x a strided
    view in a NaN buffer), conv1x1_nchw: coded and mask selectors exact, random data inside the bounds derived in tests/conv_bounds.py"""
    got = _run("direct", {} if build == "bf16" else {"MI355X_SD_DTYPE": "fp16"}, dbg=False)
    for name, v in got.items():
        print(f"{build} {name:<44} err/bound {v['ratio']:.3f} mismatch {v['mismatch']}")
        _check(name, v, build)
    assert len(got) >= 40


def test_stride2_conv_with_a_6_gib_source_takes_64_bit_addresses():
    """a stride-2 conv whose source spans more than 4 GiB passes the picker's M * lda test for the phased 256 x 256 kernel, whose buffer
    offsets are 32 bits wide: the launch must take the generic 256 x 256 loop, and the last image (behind the 4-GiB line) must be right"""
    v = _run("wide", {})["wide"]
    print(f"wide source {v['src_bytes'] / 2 ** 30:.1f} GiB: route {v['route']} err/bound {v['ratio']:.3f} rel {v['rel']:.2e}")
    assert v["src_bytes"] > 2 ** 32
    assert _route(v) == "generic/256", v["route"]
    assert v["ratio"] < 1.0, v


def test_one_pixel_image_has_no_pad_br_output():
    """bottom / right padding of a 1 x 1 image gives a 2 x 2 padded image: no 3 x 3 window fits, the entry point must say so instead of
    computing a row from a window that does not exist (C's truncating division made Ho = 1)"""
    import torch

    from paddlemix_amd import _lib, ops
    ops.init(0)
    ed = _lib.elem_dtype()
    x, w = torch.ones(2, 1, 1, 64, device="cuda", dtype=ed), torch.ones(8, 576, device="cuda", dtype=ed)
    out = torch.zeros(2, 8, device="cuda", dtype=ed)
    rc = _lib.load().mi355x_sd_conv3x3(x.data_ptr(), 64, 2, 1, 1, 64, 2, 0, w.data_ptr(), out.data_ptr(), 8, 8, None, None, 0, None, 0,
                                       1.0, _lib.PAD_BR, None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1, rc   # SD_ERR_INVALID
    assert (out == 0).all()
    with pytest.raises(ValueError):
        ops.conv3x3(x, w, None, stride=2, pad_br=True)
