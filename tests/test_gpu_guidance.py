"""-m gpu: mi355x_sd_cfg_rescale_axpby (guidance combine + guidance rescale + scheduler update in one launch, csrc/misc.hip) against
tests/guidance_bounds.py. The matrix lives in tests/guidance_child.py and runs once, in a child process under its own time limit:
every case inside the elementwise float64 bound over the whole output and bit-identical on a second launch, canaries around every
output; one launch captured in a torch.cuda.graph and replayed with two coefficient rows; the refusals; a 4-step v-prediction Euler
loop with CFG and guidance_rescale on the tiny SD config, fused against generic to the accumulated bound."""
import pytest

from tests.gpu_child import RUNNER
from tests.guidance_bounds import CASES

pytestmark = pytest.mark.gpu


def _run():
    return RUNNER.run("guidance_child.py", tag="GUIDANCE_JSON", timeout=240)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<28} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v
    assert v["ratio"] < 1.0, v                 # every element inside the float64 bound
    assert v["rerun_off"] == 0, v              # two launches, the same bits
    assert v.get("cfg_ratio", 0.0) < 1.0, v    # gr = 0: the plain guidance combine's own bound
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


def test_pipeline_fused_equals_generic():
    v = _run()["pipeline"]
    print(v)
    assert "error" not in v, v
    assert v["steps"] == 4 and v["stepped"] is None and v["finite"], v   # the fused path ran: scheduler.step was never called
    assert v["ratio"] < 1.0, v
