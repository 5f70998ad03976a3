"""-m gpu: mi355x_sd_singlestep_update (one model evaluation of DPM-Solver singlestep sampling -- guidance combine, guidance rescale,
convert_model_output, the update, the parked sample and the group's converted outputs -- in one launch, csrc/step_tail.hip
SinglestepStep) against tests/singlestep_bounds.py. The matrix lives in tests/singlestep_child.py and runs once, in a child process
under its own time limit: every case with every element of out and of the written plane inside the elementwise float64 bound, the
parked sample x's bits on an order-1 row, every other bit of the state kept, and bit-identical on a second launch, canaries around all
three; rows of order 1, order 2 with and without the plane-1 store, order 3 midpoint and heun for two prediction types, each over NaN
in the state it must not read; one captured graph node replayed over rows of order 1, 2, 3, 1 against direct launches; the refusals;
a 9-step order-3 loop with CFG on the tiny SD config, fused against generic to the accumulated bound, in the bf16 and the fp16 build.

The shapes are those of tests/test_gpu_dpm2.py (the smallest at which each kernel path can still go wrong) and so is the time limit:
400 s for the full matrix, which takes seconds; the child prints its own wall time."""
import pytest

from tests.gpu_child import RUNNER
from tests.singlestep_bounds import CASES, WRAPPED

pytestmark = pytest.mark.gpu


def _run(which="all"):
    if which == "all":
        return RUNNER.run("singlestep_child.py", tag="SINGLESTEP_JSON", timeout=400)
    return RUNNER.run("singlestep_child.py", ("pipeline",), {"MI355X_SD_DTYPE": "fp16"}, tag="SINGLESTEP_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<52} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v   # out written whole; nothing around out, P and H touched
    assert v["finite"] and v["ratio"] <= 1.0 and v["ratio_hist"] <= 1.0, v     # every element inside the float64 bound, over NaN state
    assert v["state_off"] == 0, v                          # P: x's bits at order 1; everything the row does not write: its bits
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    s = CASES[name]
    assert v["misaligned"] == ([s["misalign"]] if s.get("misalign") else []), v
    assert ("wrapper_off" in v) == (name in WRAPPED) and v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_every_order_from_a_fixed_coefficient_buffer():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"] and v["orders"] == [1.0, 2.0, 3.0, 1.0], v
    assert v["nodes"] == 1 and v["roots"] == 1 and v["edges"] == 0, v   # a single node
    assert v["replay_off"] == 0, v


def test_refusals_launch_nothing():
    v = _run()["refusals"]
    print(v)
    assert "error" not in v, v
    assert len(v) == 28 and all(v[k] == 1 for k in v if k != "touched"), v   # MI355X_SD_ERR_INVALID
    assert v["touched"] == 0, v


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_pipeline_fused_equals_generic(elem):
    got = _run("all" if elem == "bf16" else "fp16")
    v = got["pipeline"]
    print(v, "child wall time", got["seconds"], "s")
    assert "error" not in v, v
    assert v["elem"] == elem and v["launches"] == 9 and v["stepped"] == 0 and v["generic_stepped"] == 9 and v["finite"], v
    assert v["orders"] == [1, 2, 3, 1, 2, 3, 1, 2, 1] and v["generic_dtype"] == "torch.float64", v
    assert v["replay_off"] == 0, v    # the relaunched evaluations (carrying P and H through the wrapper) are the loop's own
    assert v["ratio"] <= 1.0, v
