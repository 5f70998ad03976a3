"""tests/gpu_child.py on the CPU: stand-in children that only print, sleep and exit (no GPU, no torch, no signals) drive a private
ChildRunner through every outcome -- a result, a failure, the three kinds of death -- and through run_many's fan-out."""
import os

import pytest

from tests.gpu_child import ChildRunner, Routes

# argv[1]: the counter file (one line per start); argv[2]: exit status; argv[3]: seconds to sleep first
STAND_IN = """import sys, time
open(sys.argv[1], "a").write("started\\n")
print('T_JSON {"n": 1}')
print("T_JSONX not this one")
print('T_JSON {"n": 2, "log": "%s"}' % __import__("os").environ.get("MI355X_SD_GEMM_LOG", ""), flush=True)
time.sleep(float(sys.argv[3]))
sys.exit(int(sys.argv[2]))
"""


@pytest.fixture
def child(tmp_path):
    """-> spec(name, status, sleep): run's arguments for one stand-in child, and starts(name): how often it was started"""
    script = tmp_path / "stand_in.py"
    script.write_text(STAND_IN)

    def spec(name, status=0, sleep=0.0, **kw):
        return dict(script=str(script), args=(str(tmp_path / name), str(status), str(sleep)), tag="T_JSON", timeout=60, **kw)

    def starts(name):
        return len((tmp_path / name).read_text().splitlines()) if (tmp_path / name).exists() else 0
    spec.starts = starts
    return spec


def test_success_is_the_last_tagged_line_and_runs_once(child):
    r = ChildRunner()
    assert r.run(**child("ok"))["n"] == 2
    assert r.run(**child("ok"))["n"] == 2
    assert child.starts("ok") == 1
    assert not r.dead.is_set()


def test_a_failed_child_fails_every_caller_and_runs_once(child):
    r = ChildRunner()
    for _ in range(2):
        with pytest.raises(AssertionError, match="status 1"):
            r.run(**child("bad", status=1))
    assert child.starts("bad") == 1
    assert r.run(**child("ok"))["n"] == 2   # (a failure is no death: other children still run)


@pytest.mark.parametrize("how", ["139", "134", "time limit"])
def test_a_died_child_ends_the_session_and_nothing_starts_after_it(child, how):
    r = ChildRunner()
    died = dict(child("died", sleep=5), timeout=1) if how == "time limit" else child("died", status=int(how))
    for spec in (died, died, child("healthy")):
        with pytest.raises(pytest.exit.Exception) as e:
            r.run(**spec)
        assert e.value.returncode == 3
        assert "stand_in.py" in str(e.value) and f"status {124 if how == 'time limit' else how}" in str(e.value)
    assert child.starts("died") == 1
    assert child.starts("healthy") == 0


def test_run_many_stops_starting_after_a_death(child):
    """one worker holds the dying child for 1.5 s while the other finishes healthy0 (1 s) and starts healthy1 before the death is
    seen: the event is looked at before EVERY start, so both workers stop there and healthy2 .. healthy6 never start"""
    r = ChildRunner()
    specs = [child("died", status=139, sleep=1.5)] + [child(f"healthy{i}", sleep=1) for i in range(7)]
    r.run_many(specs, workers=2)
    assert all(r._key(**s) in r.cache for s in specs)   # a recorded outcome for every spec: a dict, or None (not started)
    started = sum(child.starts(f"healthy{i}") for i in range(7))
    assert 1 <= started <= 3, started   # (2, give or take a slow process start; a worker that looked only once would start all 7)
    assert sum(r.cache[r._key(**s)] is None for s in specs) == 7 - started
    assert child.starts("died") == 1
    for s in specs:
        with pytest.raises(pytest.exit.Exception):
            r.run(**s)
    assert sum(child.starts(f"healthy{i}") for i in range(7)) == started


def test_route_log_is_set_with_the_debug_build_only(child):
    r = ChildRunner()
    assert r.run(**child("prod", route_log="MI355X_SD_GEMM_LOG"))["log"] == os.environ.get("MI355X_SD_GEMM_LOG", "")
    log = r.run(**child("dbg", dbg=True, route_log="MI355X_SD_GEMM_LOG"))["log"]
    assert os.path.basename(log) == "route.log" and log != os.environ.get("MI355X_SD_GEMM_LOG")


def test_route_log_path_is_writable_while_the_child_lives(tmp_path):
    script = tmp_path / "writer.py"
    script.write_text('import os\nopen(os.environ["MI355X_SD_NORM_LOG"], "a").write("x\\n")\nprint("W_JSON 1")\n')
    assert ChildRunner().run(str(script), tag="W_JSON", timeout=60, dbg=True, route_log="MI355X_SD_NORM_LOG") == 1


def test_routes_take_returns_the_lines_since_the_last_take(tmp_path, monkeypatch):
    log = tmp_path / "attn.log"
    monkeypatch.setenv("MI355X_SD_ATTN_LOG", str(log))
    routes = Routes("MI355X_SD_ATTN_LOG")
    assert routes.take() == []   # the file is missing
    log.write_text("a 1\nb 2\n")
    assert routes.take() == ["a 1", "b 2"]
    assert routes.take() == []
    with open(log, "a") as f:
        f.write("c 3\n")
    assert routes.take() == ["c 3"]
    monkeypatch.delenv("MI355X_SD_ATTN_LOG")
    assert Routes("MI355X_SD_ATTN_LOG").take() == []   # the variable is unset
