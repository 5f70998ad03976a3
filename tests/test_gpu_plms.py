"""-m gpu: mi355x_sd_plms_update (one model evaluation of PLMS sampling -- guidance combine, guidance rescale, the history combination,
the update, the ring of stored outputs and the parked sample -- in one launch, csrc/step_tail.hip PlmsStep) against
tests/plms_bounds.py. The matrix lives in tests/plms_child.py and runs once, in a child process under its own time limit: every case
with every element of out and of the written ring plane inside the elementwise float64 bound, the parked sample x's bits where the row
parks, every other bit of the state kept, and bit-identical on a second launch, canaries around all three; the rows of counter 0 to 6
for both prediction types (4: the ring wraps); each row over NaN in the state it must not read; one captured graph node replayed over
the rows of counter 0, 1, 2 and the wrap row against direct launches; the refusals; an 8-step (9-launch) PLMS loop with CFG on the
tiny SD config, fused against generic to the accumulated bound.

The time limit is that of tests/test_gpu_heun.py, whose child has the same shape: 400 s for the full matrix; the child prints its own
wall time."""
import pytest

from tests.gpu_child import RUNNER
from tests.plms_bounds import CASES

pytestmark = pytest.mark.gpu


def _run():
    return RUNNER.run("plms_child.py", tag="PLMS_JSON", timeout=400)


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    v = _run()[name]
    print(f"{name:<52} " + " ".join(f"{k} {v[k]:.3f}" if "ratio" in k else f"{k} {v[k]}" for k in v))
    assert "error" not in v, v
    assert v["rc"] == 0 and v["unwritten"] == 0 and v["overwritten"] == 0, v   # out written whole; nothing around out, P and H touched
    assert v["finite"] and v["ratio"] <= 1.0 and v["ratio_hist"] <= 1.0, v     # every element inside the float64 bound (NaN state included)
    assert v["state_off"] == 0, v                          # P: x's bits where the row parks; every plane the row does not write: its bits
    assert v["rerun_off"] == 0, v                          # two launches, the same bits
    s = CASES[name]
    assert v["misaligned"] == ([s["misalign"]] if s.get("misalign") else []), v
    assert v.get("wrapper_off", 0) == 0, v


def test_one_captured_node_replays_every_kind_of_row_from_a_fixed_coefficient_buffer():
    v = _run()["graph"]
    print(v)
    assert "error" not in v, v
    assert v["rc"] == 0 and v["rc_direct"] == 0 and v["finite"] and v["slots"] == [0.0, 1.0, 1.0, 0.0], v
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
    assert v["launches"] == 9 and v["stepped"] == 0 and v["generic_stepped"] == 9 and v["finite"], v
    assert v["generic_dtype"] == "torch.float64", v
    assert v["replay_off"] == 0, v    # the relaunched evaluations (carrying P and the ring through the wrapper) are the loop's own
    assert v["ratio"] <= 1.0, v
