"""-m gpu: every normalisation kernel instantiation (csrc/norm.hip, csrc/fused_ops.hip: GroupNorm split and one-launch, LayerNorm,
row statistics, RMSNorm, adaLN, adaLN + e4m3, quantize_rows, the fused adaLN + scale + residual op) against the elementwise float64
bounds of tests/norm_bounds.py over the WHOLE output of each case, on inputs that make those bounds sharp or expose the kernels'
edges: large mean offsets, 50 sigma outliers at and away from the statistics' pilot, constant, +-a and near-constant sets, rows that
make waves loop, NaN in every row gap. The case matrix lives in tests/norm_child.py and runs in a child process: once on the
debug-switch build with MI355X_SD_NORM_LOG, whose route log proves each case reached the instantiation it is named for and that the
cases together reach all 38, once on the IEEE-half build (values only)."""
import pytest

from tests.gpu_child import Family
from tests.norm_child import CASES

pytestmark = pytest.mark.gpu

# every kernel instantiation of the launchers, as "entry NCH ROWS flags" of the route log
INSTANTIATIONS = (
    ["gn_partial 0 0 x16", "gn_partial 0 0 xf32", "gn_finalize 0 0 -"]                              # gn_partial_kernel<XF32>, gn_finalize_kernel
    + [f"scale_shift_act 0 0 {a},{x}" for a in ("silu", "id") for x in ("x16", "xf32")]              # scale_shift_act_kernel<SILU, XF32>
    + ["gn_fused 0 0 silu", "gn_fused 0 0 id"]                                                        # gn_fused_kernel<SILU>
    + [f"layernorm {n} 2 {x}" for n in (2, 3, 5) for x in ("x16", "xf32")]                            # row_norm_kernel<LayerNormRows<XF32>, NCH, 2>
    + [f"row_stats {n} 4 -" for n in (1, 2, 3, 5)]                                                    # row_norm_kernel<RowStats, NCH, 4>
    + [f"rmsnorm {n} 2 -" for n in (2, 4, 8)]                                                         # rmsnorm_kernel<NCH, 2>
    + [f"adaln {n} {r} {m}" for n, r in ((2, 4), (3, 4), (5, 2)) for m in ("m16", "m32")]             # row_norm_kernel<AdaLNRows<M16>, NCH, ROWS>
    + [f"adaln_f8 {n} 1 -" for n in (2, 3, 5)]                                                        # row_norm_kernel<AdaLNF8Rows, NCH, 1>
    + ["quantize_rows 0 1 -"]                                                                         # quantize_rows_kernel
    + [f"fused_adaln {n} 1 {m}" for n in (2, 4, 8) for m in ("m16", "m32")])                          # fused_adaln_scale_residual_kernel<NCH, M16>


FAMILY = Family("norm_child.py", "NORM_JSON", "MI355X_SD_NORM_LOG", timeout=900)
_run = FAMILY.run   # every case's result on one build; the child runs once per build (a failed child is remembered, not run again per test)


def _check(name, v):
    entry, spec, _ = CASES[name]
    if spec.get("refused"):
        assert v["rc"] != 0, (name, v)          # HW * cpg / 2 one over 24576: refused, nothing written
        assert v["overwritten"] == 0, (name, v)
        return
    assert v["rc"] == 0, (name, v)
    assert v["ratio"] < 1.0, (name, v)
    assert v["unwritten"] == 0, (name, v)       # every element of the outputs written
    assert v["overwritten"] == 0, (name, v)     # no padding element, no row past the end touched
    if "ratio_resi" in v:
        assert v["ratio_resi"] < 1.0, (name, v)
    if entry == "af8":
        assert v["ratio_qs"] < 1.0 and v["ratio_l2"] < 1.0, (name, v)
    if entry in ("af8", "q8"):
        assert v["nan_bytes"] == 0, (name, v)   # no e4m3 NaN (0x7F / 0xFF) ever
    if entry == "q8":                           # the exact fp32 emulation: the scale and every byte
        assert v["exact_scale_off"] == 0 and v["exact_bytes_off"] == 0, (name, v)
    if "raw16_exact" in v:
        assert v["raw16_exact"], (name, v)      # raw16 = the 16-bit rounding of x, bit for bit
    if "exact" in v:
        assert v["exact"], (name, v)            # constant rows: y = beta / shift; RMSNorm of a zero row: 0


@pytest.mark.parametrize("name", list(CASES))
def test_case_meets_the_fp64_bound_on_its_route(name):
    v = _run("bf16")[name]
    entry, spec, route = CASES[name]
    print(f"{name:<44} err/bound {v.get('ratio', 0):.3f}  {v['route']}")
    _check(name, v)
    got = [ln.split() for ln in v["route"]]
    assert all(int(t[1]) == spec["C"] for t in got), (name, v["route"])
    assert [" ".join(t[:1] + t[2:]) for t in got] == route, (name, v["route"], route)


def test_every_norm_instantiation_is_reached():
    got = _run("bf16")
    reached = FAMILY.reached(got, lambda ln: " ".join(ln.split()[:1] + ln.split()[2:]), INSTANTIATIONS, width=28)
    assert len(INSTANTIATIONS) == 38
    assert set(INSTANTIATIONS) == reached, (sorted(set(INSTANTIATIONS) - reached), sorted(reached - set(INSTANTIATIONS)))


def test_worst_err_bound_per_family():
    """(a report: the worst err / bound of each kernel family on the debug build, what the bounds leave as headroom)"""
    got = _run("bf16")
    worst = {}
    for name, v in got.items():
        if "ratio" in v:
            e = CASES[name][0]
            worst[e] = max(worst.get(e, 0.0), v["ratio"])
    print(" ".join(f"{k} {w:.3f}" for k, w in sorted(worst.items())))
    assert all(w < 1.0 for w in worst.values()), worst


def test_fp16_build_meets_the_fp64_bound():
    """The IEEE-half build on the same matrix: the float64 bounds at u_out = 2^-10 over the whole output. (No route log in the
    production library: the debug build shares the dispatch code, and the tests above prove the routes.)"""
    got = _run("fp16")
    def check(name, v):
        print(f"fp16 {name:<44} err/bound {v.get('ratio', 0):.3f}")
        _check(name, v)

    bad = FAMILY.collect_failures(CASES, got, check)
    assert not bad, bad
