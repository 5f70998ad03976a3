"""-m gpu: mi355x_sd_dpm2_update (one model evaluation of a two-stage midpoint step, DPM2 / DPM2 a -- guidance combine, guidance
rescale, the derivative, the update, the noise term and the parked sample -- in one launch, csrc/step_tail.hip MidpointStep) against
tests/dpm2_bounds.py. The matrix lives in tests/dpm2_child.py and runs once, in a child process under its own time limit: every case
with every element of out inside the elementwise float64 bound, S exact, and bit-identical on a second launch, canaries around both;
stage 1 over a NaN S and NaN noise, stage 2 at c == 0 over NaN and null noise, stage 2 at p == 0 over a NaN x; stage 2 leaving S
untouched; one captured graph node replayed over a stage-1, a stage-2 and the next stage-1 row against direct launches; the refusals;
an 8-step (15-launch) loop of each class with CFG on the tiny SD config, fused against generic to the accumulated bound, on both
element builds.

The time limits are those of tests/test_gpu_ancestral.py, whose child has the same shape: 400 s for the full matrix, 240 s for the
pipelines alone; the child prints its own wall time."""
import pytest

from tests.dpm2_bounds import CASES
from tests.gpu_child import RUNNER

pytestmark = pytest.mark.gpu


def _run(which="all"):
    if which == "all":
        return RUNNER.run("dpm2_child.py", tag="DPM2_JSON", timeout=400)
    return RUNNER.run("dpm2_child.py", ("pipeline",), {"MI355X_SD_DTYPE": "fp16"}, tag="DPM2_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<52} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v   # out, and S: written whole in stage 1, untouched in 2
    assert v["finite"] and v["ratio"] <= 1.0, v            # every element inside the float64 bound (NaN state included)
    assert v["state_off"] == 0, v                          # stage 1: S is x bit for bit; stage 2: S keeps its bits
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    s = CASES[name]
    assert v["misaligned"] == ([s["misalign"]] if s.get("misalign") else []), v
    assert v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_both_stages_from_a_fixed_coefficient_buffer():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"] and v["stages"] == [0.0, 1.0, 0.0], v
    assert v["noisy"] == [False, True, False], v
    assert v["nodes"] == 1 and v["roots"] == 1 and v["edges"] == 0, v   # a single node
    assert v["replay_off"] == 0, v


def test_refusals_launch_nothing():
    v = _run()["refusals"]
    print(v)
    assert "error" not in v, v
    assert len(v) == 26 and all(v[k] == 1 for k in v if k != "touched"), v   # MI355X_SD_ERR_INVALID
    assert v["touched"] == 0, v


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
@pytest.mark.parametrize("sampler", ["dpm2", "dpm2a"])
def test_pipeline_fused_equals_generic(sampler, elem):
    got = _run("all" if elem == "bf16" else "fp16")
    v = got[f"pipeline {sampler}"]
    print(v, "child wall time", got["seconds"], "s")
    assert "error" not in v, v
    assert v["elem"] == elem and v["launches"] == 15 and v["stepped"] == 0 and v["generic_stepped"] == 15 and v["finite"], v
    assert v["generic_dtype"] == "torch.float64" and v["same_generator_state"], v
    assert v["noisy_rows"] == (7 if sampler == "dpm2a" else 0), v
    assert v["replay_off"] == 0, v    # the relaunched evaluations (carrying S through the wrapper) are the loop's own
    assert v["ratio"] <= 1.0, v
