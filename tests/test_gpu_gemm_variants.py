"""-m gpu: every selectable variant of the software-pipelined GEMM loops (csrc/gemm_pipe.hip) runs on the hardware in the suite, not
only the default, and the loops are held to an independent implementation: the generic loop of csrc/gemm.hip
(MI355X_SD_NO_PIPE=1). The variants change WHEN operands are staged and fetched, never the accumulation order: bit-identical."""
import pytest

from tests.gpu_child import RUNNER

pytestmark = pytest.mark.gpu
W4_REF = {"MI355X_SD_GEMM_TILE": "256", "MI355X_SD_NO_PIPE": "1", "MI355X_SD_GEMM_NO_BIAS_ACC": "1", "MI355X_SD_NO_SPLITK": "1",
          "MI355X_SD_NO_W4": "1"}


def _bar(key):   # rel-L2 of a case against its fp32 reference (16-bit stores)
    return 4e-3


def _run(env_extra):   # the A/B switches exist in the debug-switch build only; MI355X_SD_GEMM_LOG: the kernel family of every launch, per case
    return RUNNER.run("gemm_variant_child.py", (), env_extra, tag="VARIANT_JSON", timeout=600, dbg=True, route_log="MI355X_SD_GEMM_LOG")


def test_epilogue_operand_variants():
    """Round-3 epilogue forms (csrc/gemm_epilogue.h): residual fetched during the last K iterations, a row-tile's operands fetched in
    one batch, bias as the accumulators' initial value. The first two change WHEN operands are loaded, never the arithmetic:
    bit-identical to the group-at-a-time epilogue. The bias moves from the end of the fp32 sum to its start: same tolerance."""
    base = _run({})
    for k, v in base.items():
        assert v["rel"] < _bar(k), (k, v)
    for env in ({"MI355X_SD_GEMM_NO_PRE": "1"}, {"MI355X_SD_GEMM_NO_EPI_BATCH": "1"},
                {"MI355X_SD_GEMM_NO_PRE": "1", "MI355X_SD_GEMM_NO_EPI_BATCH": "1"},
                {"MI355X_SD_GEMM_PERSIST": "0"}):   # one block per tile instead of persistent blocks walking several
        got = _run(env)
        for k in base:
            assert got[k]["sha"] == base[k]["sha"], (env, k, got[k], base[k])
    got = _run({"MI355X_SD_GEMM_NO_BIAS_ACC": "1"})
    for k, v in got.items():
        assert v["rel"] < _bar(k), (k, v)


def test_small_tile_ring_is_bit_identical_to_the_128_tile_without_slices():
    """csrc/gemm_small.hip (round 6): the 64 x 64 tile with the six-stage ring that the small launches of a batch-1 step take instead
    of split-K slices + a reduce kernel. Against the 128 x 128 tiles walking the same K in one chain (MI355X_SD_NO_SPLITK on both
    sides, MI355X_SD_NO_SMALL on the reference's): another tile, another ring depth, the same products in the same order -> the same
    bits on every case of the child (ragged M / N, one to 35 K-tiles, residual rows inside a wider buffer, GEGLU, LayerNorm-free).
    Against the sliced form it replaces the sums associate differently: equal within the kernels' tolerance (the child's rel)."""
    new = _run({"MI355X_SD_NO_SPLITK": "1"})
    ref = _run({"MI355X_SD_NO_SPLITK": "1", "MI355X_SD_NO_SMALL": "1"})
    for k, v in new.items():
        assert v["rel"] < _bar(k), (k, v)
        assert v["sha"] == ref[k]["sha"], (k, v, ref[k])
    sliced = _run({"MI355X_SD_NO_SMALL": "1"})
    assert any(sliced[k]["sha"] != v["sha"] for k, v in _run({}).items())   # (the picker does take the small tile somewhere)


@pytest.mark.parametrize("tile_map", ["160:129", "257:129,320:129"])
def test_four_wave_tiles(tile_map):
    """The four-wave tiles built for two co-resident blocks per CU (gemm_cfg.h: 128x160) substituted for the
    picker's choice: every output element still accumulates its K products in the same order -> bit-identical."""
    base = _run({})
    got = _run({"MI355X_SD_GEMM_TILE_MAP": tile_map})
    for k in base:
        assert got[k]["rel"] < _bar(k), (tile_map, k, got[k])
        # same loop, other tile: bit-identical. (Launches the picker gives to the phased 256x256 kernel, id 257, walk K in another
        # order: equal within the tolerance only.)
        if "257" not in tile_map:
            assert got[k]["sha"] == base[k]["sha"], (tile_map, k, got[k], base[k])


@pytest.mark.parametrize("tile_env", [{}, {"MI355X_SD_GEMM_TILE": "320"}, {"MI355X_SD_GEMM_TILE": "128"}, {"MI355X_SD_GEMM_TILE": "129"},
                                      {"MI355X_SD_GEMM_TILE": "160"}, {"MI355X_SD_GEMM_TILE": "256"}, {"MI355X_SD_GEMM_TILE": "258"},
                                      {"MI355X_SD_GEMM_TILE": "259"}],
                         ids=["picker", "256x320", "128x128", "128x160", "256x160", "256x256-pipelined", "256x256-four-waves", "256x160-four-waves"])
def test_pipelined_loops_are_bit_identical_to_the_generic_loop(tile_env):
    """The interleaved register-pipelined loop (round 4: one LDS-DMA piece / one fragment read between MFMA pairs, the A and W
    pieces of a tile issued in different half-iterations, unrolled tail or -- early-residual kernels -- a tail loop, static vmcnt)
    and the streaming loop against the plain double-buffered loop of csrc/gemm.hip on every tile family: another schedule, another
    author's-week of code, the same tiles and the same K order -> the same bits. (Bias added in the epilogue on both sides: the
    pipelined kernels otherwise start their accumulators at the bias.) Covers two and three LDS stages, the early-residual
    kernels, GEGLU, ragged M / N, launches of 1 .. 5 K-tiles (the tail alone), split-K slices and the implicit-GEMM convs.
    The same comparison held the interleaved loop to the round-3 burst loop before that was deleted (profiles/r04_s2_tests.txt)."""
    ref = _run(dict(tile_env, MI355X_SD_NO_PIPE="1", MI355X_SD_GEMM_NO_BIAS_ACC="1"))
    new = _run(dict(tile_env, MI355X_SD_GEMM_NO_BIAS_ACC="1"))
    # MI355X_SD_NO_PIPE does not reach the four-wave tile (launch_gemm takes it before the pipelined loops, and a forced tile returns
    # from pick_tile before MI355X_SD_NO_W4 is read): the launches that ran it (route log) are held to the generic 256 x 256 loop with
    # the four-wave tile off instead -- the same K order, the bias after the sum (tests/test_gpu_gemm_w4.py has its own case matrix)
    w4_ref = _run(W4_REF)
    w4 = [k for k, v in new.items() if any(r.split()[-1].startswith("w4/") for r in v["route"])]
    if tile_env.get("MI355X_SD_GEMM_TILE") in ("258", "259") or not tile_env:
        assert w4, (tile_env, "no launch reached the four-wave tile")
    for k, v in new.items():
        assert v["rel"] < _bar(k), (tile_env, k, v)
        if k in w4 and any(r.split()[-1].endswith("+ws") for r in v["route"]):
            # (widened e4m3: the four-wave epilogue fuses scale and bias into one FMA where the generic loop rounds twice --
            # tests/test_gpu_gemm_w4.py WS_NOTE -- so the four-wave tile of the other width is the bit-exact reference)
            other = _run({"MI355X_SD_GEMM_TILE": "258" if tile_env.get("MI355X_SD_GEMM_TILE") == "259" else "259",
                          "MI355X_SD_GEMM_NO_BIAS_ACC": "1"})
            if any(r.split()[-1].startswith("w4/") for r in other[k]["route"]):
                assert v["sha"] == other[k]["sha"], (tile_env, k, v, other[k])
        elif k in w4:
            assert not any(r.split()[-1].startswith("w4/") for r in w4_ref[k]["route"]), (k, w4_ref[k]["route"])
            assert v["sha"] == w4_ref[k]["sha"], (tile_env, k, v, w4_ref[k])
        else:
            assert v["sha"] == ref[k]["sha"], (tile_env, k, v, ref[k])
