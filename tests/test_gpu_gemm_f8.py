"""-m gpu: the W8A8 fp8-MFMA GEMM -- gemm256_kernel's F8 instantiation with gemm_epilogue_f8, through mi355x_sd_linear_f8 and
mi355x_sd_linear_f8_q -- held to exact bits and to an elementwise float64 bound over its whole output.

The case matrix of tests/gemm_f8_child.py runs once in the bf16 production library and once in the IEEE-half build. Class 1 requires
bit equality with a reference whose every intermediate is exactly representable (no model of the instruction: pure indexing); class
2 requires every element inside the bound of tests/gemm_f8_bounds.py and the rel-L2 bar the project already uses for these stores;
the e4m3 output must have its row scale within 4 * 2^-24 and every byte inside its interval of accepted codes. Every output sits in
a canary buffer, every input gap holds NaN (0x7F in the e4m3 operands): nothing unwritten, nothing overwritten. The launches the
entries must refuse return a non-zero status and write nothing. Each launch without a row remap is repeated through the ops wrapper
on compact operands and must give the same bits."""
import pytest

from tests.gemm_f8_bounds import MULTI_CAP
from tests.gemm_f8_child import CASES
from tests.gpu_child import RUNNER, Family

pytestmark = pytest.mark.gpu
REL_BAR = {"bf16": 4e-3, "fp16": 6e-4}   # the rel-L2 bars of tests/test_gpu_gemm_linear.py
BUILDS = {"bf16": {}, "fp16": {"MI355X_SD_DTYPE": "fp16"}}


# (a child: library load + ~300 launches of at most 1 GFLOP + their float64 references on the device: seconds)
CHILD = Family("gemm_f8_child.py", "F8_JSON", None, timeout=300)


def _spec(build):
    return CHILD.spec((), BUILDS[build])


def _run(build):
    """the child's JSON in one build; the first call starts both children, each under its own time limit (tests/gpu_child.py)"""
    RUNNER.run_many([_spec(b) for b in BUILDS], workers=2)
    return RUNNER.run(**_spec(build))


def _names(cls):
    return [n for n, s in CASES.items() if s["cls"] == cls]


def _line(build, k, v):
    parts = [f"{build:>4} {k:<28}"]
    if "ratio" in v:
        parts.append(f"err/bound {v['ratio']:.3f} rel {v['rel']:.2e}")
    if "off" in v:
        parts.append(f"differing {v['off']}")
    if "scale_ratio" in v:
        parts.append(f"scale {v['scale_ratio']:.3f} outside {v['outside']} nan {v['nan']} multi {v['multi']:.4f}")
    parts.append(f"unwritten {v.get('unwritten', 0)} overwritten {v['overwritten']} wrapper {v.get('wrapper_off', '-')}")
    print("  ".join(parts))


def _written(build, k, v):
    assert v["rc"] == 0, (build, k, v)
    assert v["unwritten"] == 0 and v["overwritten"] == 0, (build, k, v)
    assert v.get("wrapper_off", 0) == 0, (build, k, v)


def _e4m3(build, k, v):
    _written(build, k, v)
    assert ("wrapper_off" in v) == (CASES[k]["N"] % 8 == 0), (build, k, v)   # (the wrapper's ldc is N)
    assert v["scale_ratio"] <= 1.0, (build, k, v)               # |c_scale - s64| <= 4 * 2^-24 * s64, rows >= M untouched
    assert v["outside"] == 0 and v["nan"] == 0, (build, k, v)   # every byte inside its interval of accepted codes, none NaN
    assert v["multi"] <= MULTI_CAP, (build, k, v)


@pytest.mark.parametrize("build", list(BUILDS))
def test_no_case_is_skipped(build):
    got = _run(build)
    assert set(got) == set(CASES), sorted(set(CASES) ^ set(got))


@pytest.mark.parametrize("build", list(BUILDS))
def test_class_1_exact_bits(build):
    """small-integer operands, power-of-two scales or integer epilogue operands: every output bit is known, off == 0. Both
    mirrors, every edge shape, both remaps from both base pointers; the same operands through the e4m3 output."""
    got = _run(build)
    names = _names("exact")
    assert len(names) == 2 * (30 + 6 + 1 + 4)
    for k in names:
        v = got[k]
        _line(build, k, v)
        if "q" in v:
            _line(build, k + " -> e4m3", v["q"])
    for k in names:
        v = got[k]
        _written(build, k, v)
        assert v["off"] == 0, (build, k, v)
        assert ("wrapper_off" in v) == ("a-remap" not in k), (build, k, v)
        assert ("q" in v) == bool(CASES[k].get("q")), (build, k, v)
        if "q" in v:
            _e4m3(build, k, v["q"])


@pytest.mark.parametrize("build", list(BUILDS))
def test_class_2_float64_bound(build):
    """dense operands quantised as the model does, every epilogue form: err / bound < 1 on every element, rel-L2 inside the bar"""
    got = _run(build)
    names = _names("dense")
    assert len(names) == 4 * 6
    for k in names:
        _line(build, k, got[k])
    print(f"{build}: worst err/bound {max((got[k]['ratio'], k) for k in names)}")
    for k in names:
        v = got[k]
        _written(build, k, v)
        assert v["ratio"] < 1.0, (build, k, v)
        assert v["rel"] < REL_BAR[build], (build, k, v)


@pytest.mark.parametrize("build", list(BUILDS))
def test_class_2_e4m3_output(build):
    """mi355x_sd_linear_f8_q: the row scale, the interval rule, the multi-code cap; 8-byte stores and the 4-byte tail (N = 12)"""
    got = _run(build)
    names = _names("denseq")
    assert len(names) == 4 * 2
    for k in names:
        _line(build, k, got[k])
    for k in names:
        _e4m3(build, k, got[k])


@pytest.mark.parametrize("build", list(BUILDS))
def test_refused_launches_return_a_status_and_write_nothing(build):
    got = _run(build)
    names = _names("refuse")
    assert len(names) == 10
    for k in names:
        v = got[k]
        print(f"{build:>4} {k:<28} status {v['rc']} overwritten {v['overwritten']}")
        assert v["rc"] != 0 and v["overwritten"] == 0, (build, k, v)
    assert got["refuse K%128"]["wrapper_raises"] is True   # MI355XError through ops.linear_f8
