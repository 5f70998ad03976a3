"""-m gpu: mi355x_sd_ancestral_update (one ancestral Euler step -- guidance combine, guidance rescale, prev = a x + b e + c z -- in
one launch, csrc/misc.hip) against tests/ancestral_bounds.py. The matrix lives in tests/ancestral_child.py and runs once, in a child
process under its own time limit: every case with every element inside the elementwise float64 bound and bit-identical on a second
launch, canaries around out; the c = 0 row over a NaN plane and over a null one; one captured graph node replayed over three
consecutive rows with the noise rewritten in place against three direct launches; the refusals; an 8-step Euler a loop with CFG and
guidance_rescale on the tiny SD config under one device generator seed, fused against generic to the accumulated bound, on both
element types (the IEEE-half build in a second child).

The time limits are those of tests/test_gpu_multistep.py, whose child has the same shape: 400 s for the full matrix, 240 s for the
pipeline alone; the children print their own wall time."""
import pytest

from tests.ancestral_bounds import CASES
from tests.gpu_child import RUNNER

pytestmark = pytest.mark.gpu


def _run(which="all"):
    if which == "all":
        return RUNNER.run("ancestral_child.py", tag="ANCESTRAL_JSON", timeout=400)
    return RUNNER.run("ancestral_child.py", ("pipeline",), {"MI355X_SD_DTYPE": "fp16"}, tag="ANCESTRAL_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<44} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v
    assert v["finite"] and v["ratio"] <= 1.0, v            # every element inside the float64 bound (a NaN plane at c = 0 included)
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    s = CASES[name]
    want = {"z": "z", "x": "x", "eu": "eu", "et": "et", "out": "out"}.get(s.get("misalign"))
    assert v["misaligned"] == ([want] if want else []), v
    assert v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_three_rows_with_the_noise_rewritten_in_place():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"] and v["last_c"] == 0.0, v
    assert v["nodes"] == 1 and v["roots"] == 1 and v["edges"] == 0, v   # a single node
    assert v["replay_off"] == 0, v


def test_refusals_launch_nothing():
    v = _run()["refusals"]
    print(v)
    assert "error" not in v, v
    assert all(v[k] == 1 for k in v if k != "touched"), v   # MI355X_SD_ERR_INVALID
    assert v["touched"] == 0, v


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_pipeline_fused_equals_generic(elem):
    got = _run("all" if elem == "bf16" else "fp16")
    v = got["pipeline"]
    print(v, "child wall time", got["seconds"], "s")
    assert "error" not in v, v
    assert v["elem"] == elem and v["steps"] == 8 and v["stepped"] == 0 and v["generic_stepped"] == 8 and v["finite"], v
    assert v["last_c"] == 0.0 and v["same_generator_state"], v
    assert v["replay_off"] == 0, v    # the relaunched steps (on the planes redrawn from the seed) are the loop's own
    assert v["ratio"] <= 1.0, v
