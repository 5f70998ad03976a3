"""-m gpu: mi355x_sd_unipc_update (one UniPC step -- guidance combine, guidance rescale, convert_model_output, corrector, predictor,
last_sample and the history shift -- in one launch, csrc/misc.hip) against tests/unipc_bounds.py. The matrix lives in
tests/unipc_child.py and runs once, in a child process under its own time limit: every case with out, last and history plane 0 inside
the elementwise float64 bound, the shifted planes bit-exact, everything bit-identical on a second launch, canaries around every
buffer the kernel writes; one captured graph node replayed over three consecutive rows against three direct launches; the refusals;
an 8-step third-order loop with CFG and guidance_rescale on the tiny SD config, fused against generic to the accumulated bound, on both
element types (the IEEE-half build in a second child).

The time limits are those of tests/test_gpu_multistep.py, whose child has the same shape: 400 s for the 25 entries of the full
matrix, 240 s for the pipeline alone; the children print their own wall time."""
import pytest

from tests.gpu_child import RUNNER
from tests.unipc_bounds import CASES

pytestmark = pytest.mark.gpu


def _run(which="all"):
    if which == "all":
        return RUNNER.run("unipc_child.py", tag="UNIPC_JSON", timeout=400)
    return RUNNER.run("unipc_child.py", ("pipeline",), {"MI355X_SD_DTYPE": "fp16"}, tag="UNIPC_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<44} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v
    assert v["ratio"] <= 1.0 and v["ratio_last"] <= 1.0 and v["ratio_plane0"] <= 1.0, v   # every element inside the float64 bound
    assert v["shift_off"] == 0, v                          # planes 1 and 2 are the old planes 0 and 1, bit for bit
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    assert v["misaligned"] == int(bool(CASES[name].get("misalign"))), v
    assert v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_a_loop_with_fixed_pointers():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"], v
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
    assert v["elem"] == elem and v["steps"] == 8 and v["stepped"] is None and v["generic_stepped"] == 8 and v["finite"], v
    assert v["replay_off"] == 0, v    # the relaunched steps (whose last and hist are the state the bound uses) are the loop's own
    assert v["ratio"] <= 1.0, v
