"""-m gpu: every 16-bit linear GEMM kernel family against float64 math, over the whole output.

tests/test_gpu_gemm_variants.py proves that the kernel families give each other's bits; what all of them share -- gemm_epilogue.h, the
generic loop the others are compared with -- is held here to the elementwise bound of tests/gemm_bounds.py, family by family, on the
case matrix of tests/gemm_linear_child.py: the generic loop on its four tiles (also with e4m3 weight bytes and with the LayerNorm
fold), split-K slices + the reduce kernel, the pipelined loops with the early-residual kernel and its refusals, the 128 x 160 tile,
the phased 256 x 256 kernel, the small tile, the picker in the production library and in the fp16 build. Each family is reached by a
forced tile of the debug-switch build, and the MI355X_SD_GEMM_LOG route of every case must be exactly the one the child's table
expects: a launch that falls back to another kernel fails. Where two families walk K in the same order the same bits are required."""
import pytest

from tests.gemm_linear_child import COMMON, GENERIC_OF, SWITCHES, expected_route, names_of
from tests.gpu_child import RUNNER, Family

pytestmark = pytest.mark.gpu
REL_BAR = {"bf16": 4e-3, "fp16": 6e-4}   # the rel-L2 bars of tests/test_gpu_gemm_variants.py and tests/test_gpu_fp16.py
PROD = {"prod": {}, "fp16": {"MI355X_SD_DTYPE": "fp16"}}   # the production libraries: no switches, no route log


# (a child: library load + ~50 launches of at most a few GFLOP + their float64 references: seconds)
CHILD = Family("gemm_linear_child.py", "LINEAR_JSON", "MI355X_SD_GEMM_LOG", timeout=240)


def _spec(sw):
    dbg = sw not in PROD
    return CHILD.spec(names_of(sw) if dbg else (), (SWITCHES if dbg else PROD)[sw], dbg)


def _run(sw):
    """the child's JSON under switch set sw. The children are independent processes (the switches are read once per process); the
    first call starts all of them, four at a time, each under its own time limit; after a child that died on the GPU none is started
    and the session ends (tests/gpu_child.py)."""
    RUNNER.run_many([_spec(s) for s in list(SWITCHES) + list(PROD)], workers=4)
    return RUNNER.run(**_spec(sw))


def _check(sw, got, names, fp16=False):
    assert set(names) <= set(got), (sw, sorted(set(names) - set(got)))   # no case skipped
    for k in names:
        v = got[k]
        print(f"{sw:>8} {k:<18} err/bound {v['ratio']:.3f}  rel {v['rel']:.2e}  guard {v['guard']}  {v['route']}")
        assert v["ratio"] < 1.0, (sw, k, v)
        assert v["rel"] < REL_BAR["fp16" if fp16 else "bf16"], (sw, k, v)
        assert v["guard"] in (None, 0), (sw, k, v)   # canary rows / columns untouched


def _route(v):
    assert len(v["route"]) == 1, v["route"]   # one launch per case
    return v["route"][0].split()[-1]


@pytest.mark.parametrize("sw", [s for s in SWITCHES if not s.endswith("one")])
def test_family_meets_the_fp64_bound_on_its_exact_route(sw):
    """Every case under one switch set: inside the float64 bound over the whole output, inside the rel-L2 bar, guard bands intact,
    and on exactly the kernel family the table names (generic/<tile>[+f8|+ln][+splitk], pipe/<tile>[+splitk], gemm256[+ln], small)."""
    got, names = _run(sw), names_of(sw)
    _check(sw, got, names)
    for k in names:
        assert _route(got[k]) == expected_route(k, sw), (sw, k, got[k]["route"], expected_route(k, sw))


def test_every_family_is_reached():
    """the table itself: every family of the issue appears among the asserted routes (tests/test_gemm_linear_table.py checks the
    table against the dispatch conditions and each family's ragged-M / ragged-N / epilogue coverage, on the CPU)"""
    seen = {expected_route(k, sw) for sw in SWITCHES for k in names_of(sw)}
    want = {f"generic/{t}{f}" for t in (128, 160, 256, 320) for f in ("", "+ln", "+f8")}
    want |= {"generic/128+splitk", "generic/128+ln+splitk", "generic/128+f8+splitk", "pipe/128+splitk", "gemm256", "gemm256+ln", "small"}
    want |= {f"pipe/{t}" for t in (128, 129, 160, 320, 256)}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("sw", sorted(GENERIC_OF))
def test_pipelined_tile_has_the_bits_of_its_generic_configuration(sw):
    """bias after the sum, one chain over K (MI355X_SD_GEMM_NO_BIAS_ACC, MI355X_SD_NO_SPLITK): the pipelined loop of a tile -- the
    early-residual kernel included, which a launch without a bias still takes -- and the generic loop sum the same products in the
    same order. (The 128 x 160 tile has no generic configuration of its own: the generic 128 x 128 loop.)"""
    new, ref = _run(sw), _run(GENERIC_OF[sw])
    for k in names_of(GENERIC_OF[sw]):
        assert new[k]["sha"] == ref[k]["sha"], (sw, k, new[k], ref[k])


def test_small_tile_and_sliced_forms_have_their_references_bits():
    """the small tile against the pipelined 128 tile without slices (both start the accumulators at the bias); split-K slices of
    the pipelined loop against those of the generic loop (both add the bias in the reduce kernel)"""
    small, ref = _run("pick"), _run("p128ns")
    n = 0
    for k in names_of("pick"):
        if expected_route(k, "pick") == "small":
            assert small[k]["sha"] == ref[k]["sha"], (k, small[k], ref[k])
            n += 1
    assert n >= 30
    pipe, gen = _run("p128"), _run("g128sk")
    deep = [k for k in names_of("g128sk") if "+splitk" in expected_route(k, "p128") and expected_route(k, "p128").startswith("pipe")]
    assert len(deep) >= 2
    for k in deep:
        assert pipe[k]["sha"] == gen[k]["sha"], (k, pipe[k], gen[k])


@pytest.mark.parametrize("tile", ["128", "129", "160", "320", "256"])
def test_persistent_blocks_have_the_bits_of_one_block_per_tile(tile):
    """a few more tiles than pipe_grid_x's cap (persistent blocks walk two tiles, most walk one) against MI355X_SD_GEMM_PERSIST=0"""
    name = f"persist {tile}"
    one = _run(f"p{tile}one")
    _check(f"p{tile}one", one, [name])
    assert _route(one[name]) == f"pipe/{tile}", one[name]["route"]
    assert _run(f"p{tile}")[name]["sha"] == one[name]["sha"], (name, one[name])


@pytest.mark.parametrize("lib", list(PROD))
def test_picker_in_the_production_libraries(lib):
    """no switches, no route log: whatever the picker gives the common cases in the bf16 production library and in the IEEE-half
    build (u_out = 2^-10, rel-L2 6e-4)"""
    _check(lib, _run(lib), COMMON, fp16=lib == "fp16")
