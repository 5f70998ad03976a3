"""-m gpu: mi355x_sd_multistep_update (one DPM-Solver multistep step -- guidance combine, guidance rescale, convert_model_output,
update and history -- in one launch, csrc/misc.hip) against tests/multistep_bounds.py. The matrix lives in tests/multistep_child.py
and runs once, in a child process under its own time limit: every case with both outputs inside the elementwise float64 bound and
bit-identical on a second launch, canaries around both outputs; one launch captured in a torch.cuda.graph and replayed with a
second-order and a first-order coefficient row; the refusals; a 6-step dpmsolver++ loop with CFG and guidance_rescale on the tiny SD
config, fused against generic to the accumulated bound, on both element types (the IEEE-half build in a second child).

The time limit is that of tests/test_gpu_guidance.py for its 14 entries (240 s) scaled to the 24 entries here: 400 s; the children
print their own wall time (measured on the MI355X: 1.2 s after the imports for the full matrix, 0.4 s for the pipeline
alone)."""
import pytest

from tests.gpu_child import RUNNER
from tests.multistep_bounds import CASES

pytestmark = pytest.mark.gpu


def _run(which="all"):
    if which == "all":
        return RUNNER.run("multistep_child.py", tag="MULTISTEP_JSON", timeout=400)
    return RUNNER.run("multistep_child.py", ("pipeline",), {"MI355X_SD_DTYPE": "fp16"}, tag="MULTISTEP_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<36} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v
    assert v["ratio"] < 1.0 and v["ratio_m"] < 1.0, v     # every element of out and m_out inside the float64 bound
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    assert v["misaligned"] == int(bool(CASES[name].get("misalign"))), v
    assert v.get("wrapper_off", 0) == 0, v


def test_captured_graph_replays_with_per_step_coefficients():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["ratio"] < 1.0, v
    assert v["nodes"] >= 1 and v["roots"] == 1 and v["edges"] == v["nodes"] - 1, v   # a single branch


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
    assert v["elem"] == elem and v["steps"] == 6 and v["stepped"] is None and v["generic_stepped"] == 6 and v["finite"], v
    assert v["replay_off"] == 0, v    # the relaunched steps (whose m_out is the history the bound uses) are the loop's own
    assert v["ratio"] < 1.0, v
