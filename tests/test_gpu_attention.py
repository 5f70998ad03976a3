"""-m gpu: every attention kernel form launch_dp launches (csrc/attention.hip) against the elementwise float64 bound of
tests/attn_bounds.py, on the inputs of tests/attn_cases.py that make that bound sharp (uniform keys, one-hot selectors, bias
selectors, Skv = 1, random data), over the WHOLE output of each case. The case matrix lives in tests/attn_child.py and runs in a
child process: once on the debug-switch build with MI355X_SD_ATTN_LOG, whose route log proves each case reached the kernel it is
named for and that the cases together reach every instantiation, once on the IEEE-half build (values only)."""
import pytest

from tests.attn_child import CASES
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu

# every kernel instantiation launch_dp can launch, by its route-log name (the debug build's timing form of the 16x16x32 kernel,
# MI355X_SD_ATTN_STAMP, excepted: it is the m16+log2 kernel writing clock stamps into q)
INSTANTIATIONS = [
    "short/1", "short/2", "short/3", "short/4", "short/1+log2", "short/2+log2", "short/3+log2", "short/4+log2",   # attention_short_kernel
    "flash64/qt2", "flash64/qt2+log2",               # attention_kernel<64, false, 2, 0 | 3>
    "m16", "m16+log2",                               # attention16_kernel<false | true>
    "flash64+lazy", "flash64+lazy+wide", "flash64+log2", "flash64+log2+wide",   # attention_kernel<64, false, 1, 1 | 5 | 3 | 7>
    "flash64+bias",                                  # attention_kernel<64, true, 1, 0>
    "flash96", "flash96+bias", "flash160", "flash160+bias",   # attention_kernel<96 | 160, false | true, 1, 0>
]


NOM16 = [n for n in CASES if n.startswith("nom16")]


FAMILY = Family("attn_child.py", "ATTN_JSON", "MI355X_SD_ATTN_LOG", timeout=900)


def _run(dtype):
    """every case's result; a child runs once (tests/gpu_child.py: a failed child is remembered, not run again per test)"""
    if dtype == "bf16":
        got = FAMILY.run("bf16", [n for n in CASES if n not in NOM16])
        return dict(got, **FAMILY.run("bf16", NOM16, {"MI355X_SD_ATTN_NO_M16": "1"}))   # (started only after the first child gave its result)
    return FAMILY.run(dtype)


def _check(name, v, rel_bar):
    spec = CASES[name][0]
    assert v["ratio"] < 1.0, (name, v)
    if spec["kind"] == "S4":
        assert v["rel"] < rel_bar, (name, v)
    assert v["unwritten"] == 0, (name, v)      # every element of the view written
    assert v["overwritten"] == 0, (name, v)    # no padding element touched
    if spec["kind"] == "S3" and spec["accum"] is None:
        assert v["same_v"], (name, v)          # one key: out == v bit for bit
    if spec["ninf"]:
        assert v["zero_rows"], (name, v)       # a row masked entirely with -inf: 0


@pytest.mark.parametrize("name", list(CASES))
def test_case_meets_the_fp64_bound_on_its_route(name):
    v = _run("bf16")[name]
    spec, fam, _ = CASES[name]
    print(f"{name:<36} err/bound {v['ratio']:.3f}  rel {v['rel']:.2e}  {v['route']}")
    _check(name, v, 5e-3)
    assert len(v["route"]) == 1, v["route"]   # one launch per case
    want = f"{spec['B']} {spec['H']} {spec['Sq']} {spec['Skv']} {spec['D']} {fam}"
    assert v["route"][0] == want, (name, v["route"], want)


def test_every_launch_dp_instantiation_is_reached():
    got = _run("bf16")
    reached = FAMILY.reached(got, lambda ln: ln.split()[-1], INSTANTIATIONS, width=20)
    assert set(INSTANTIATIONS) <= reached, sorted(set(INSTANTIATIONS) - reached)
    assert reached <= set(INSTANTIATIONS), sorted(reached - set(INSTANTIATIONS))


def test_fp16_build_meets_the_fp64_bound():
    """The IEEE-half build on the same matrix: the float64 bound at u_out = 2^-10, u_p = 2^-11 over the whole output. (No route log
    in the production library: the debug build shares the dispatch code, and the tests above prove the routes.)"""
    got = _run("fp16")
    def check(name, v):
        print(f"fp16 {name:<36} err/bound {v['ratio']:.3f}  rel {v['rel']:.2e}")
        _check(name, v, 6e-4)   # (fp16 bar of tests/test_gpu_fp16.py: fp32 accumulation, one fp16 rounding)

    bad = FAMILY.collect_failures(CASES, got, check)
    assert not bad, bad
