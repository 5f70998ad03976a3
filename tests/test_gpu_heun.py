"""-m gpu: mi355x_sd_heun_update (one model evaluation of a two-stage Heun step -- guidance combine, guidance rescale, the derivative,
the update and the parked state -- in one launch, csrc/step_tail.hip HeunStep) against tests/heun_bounds.py. The matrix lives in
tests/heun_child.py and runs once, in a child process under its own time limit: every case with every element of out, S and D
inside the elementwise float64 bound (S exact) and bit-identical on a second launch, canaries around all three; stage 1 over NaN
state and stage 2 at g == 0 over a NaN derivative; stage 2 leaving S and D untouched; one captured graph node replayed over a
stage-1, a stage-2 and the next stage-1 row against direct launches; the refusals; an 8-step (15-launch) Heun loop with CFG on the
tiny SD config, fused against generic to the accumulated bound.

The time limit is that of tests/test_gpu_ancestral.py, whose child has the same shape: 400 s for the full matrix; the child prints its
own wall time."""
import pytest

from tests.gpu_child import RUNNER
from tests.heun_bounds import CASES

pytestmark = pytest.mark.gpu


def _run():
    return RUNNER.run("heun_child.py", tag="HEUN_JSON", timeout=400)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<48} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v   # out, and S / D: written whole in stage 1, untouched in 2
    assert v["finite"] and v["ratio"] <= 1.0 and v["ratio_D"] <= 1.0, v    # every element inside the float64 bound (NaN state included)
    assert v["state_off"] == 0, v                          # stage 1: S is x bit for bit; stage 2: S and D keep their bits
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    s = CASES[name]
    assert v["misaligned"] == ([s["misalign"]] if s.get("misalign") else []), v
    assert v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_both_stages_from_a_fixed_coefficient_buffer():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"] and v["stages"] == [0.0, 1.0, 0.0], v
    assert v["nodes"] == 1 and v["roots"] == 1 and v["edges"] == 0, v   # a single node
    assert v["replay_off"] == 0, v


def test_refusals_launch_nothing():
    v = _run()["refusals"]
    print(v)
    assert "error" not in v, v
    assert all(v[k] == 1 for k in v if k != "touched"), v   # MI355X_SD_ERR_INVALID
    assert v["touched"] == 0, v


def test_pipeline_fused_equals_generic():
    got = _run()
    v = got["pipeline"]
    print(v, "child wall time", got["seconds"], "s")
    assert "error" not in v, v
    assert v["launches"] == 15 and v["stepped"] == 0 and v["generic_stepped"] == 15 and v["finite"], v
    assert v["generic_dtype"] == "torch.float64", v
    assert v["replay_off"] == 0, v    # the relaunched evaluations (carrying S and D through the wrapper) are the loop's own
    assert v["ratio"] <= 1.0, v
