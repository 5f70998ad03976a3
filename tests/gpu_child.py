"""The one runner of the GPU tests' child processes, and what the children share.

Parent side (the test files): RUNNER.run starts tests/<script> as a fresh process under the caller's time limit, once per
(script, args, env_extra, dbg), and remembers every outcome. A child that DIED on the GPU -- a signal, an abort (134), a segmentation
fault (139), a time limit (124, 137) -- ends the pytest session with status 3 and nothing is started after it, by any test file:
RUNNER is shared. A child that merely failed (a Python exception) fails every test that asks for it and is not run again.

Child side: Routes (the route-log reader), emit (the tagged JSON line the parent parses), sha (an output's bits)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def died(rc):
    return rc < 0 or rc in (124, 134, 137, 139)   # a signal, a time limit, an abort, a segmentation fault


class ChildRunner:
    def __init__(self):
        self.cache = {}                 # key -> dict(rc, out, err, dt[, json]), or None: not started, a child had died
        self.dead = threading.Event()   # set by the thread that sees a child die: from then on no child is started
        self.dead_msg = None

    @staticmethod
    def _key(script, args=(), env_extra=None, *, dbg=False, tag=None, timeout=None, route_log=None):   # (run's arguments)
        return (script, tuple(args), tuple(sorted((env_extra or {}).items())), dbg)

    def _start(self, script, args=(), env_extra=None, *, timeout, dbg=False, route_log=None, tag=None):
        """one child -> dict(rc, out, err, dt), or None (nothing started) once a child has died. A child that exceeds its time limit
        counts as dead (status 124)."""
        if self.dead.is_set():
            return None
        t0 = time.time()
        with tempfile.TemporaryDirectory() as td:
            env = dict(os.environ, **(env_extra or {}))
            if dbg:   # (the switches and the route logs exist in the debug-switch build only)
                env["MI355X_SD_LIB"] = "dbg"
                if route_log:
                    env[route_log] = os.path.join(td, "route.log")
            else:     # (the production library, whatever the caller's own environment selects)
                env.pop("MI355X_SD_LIB", None)
            try:
                p = subprocess.run([sys.executable, os.path.join(TESTS, script), *args], env=env, cwd=ROOT, capture_output=True,
                                   text=True, timeout=timeout)
                got = dict(rc=p.returncode, out=p.stdout, err=p.stderr)
            except subprocess.TimeoutExpired as e:
                got = dict(rc=124, out="", err=f"time limit: {e}")
        if died(got["rc"]):
            self.dead_msg = f"{script} {list(args)} {env_extra or {}} died with status {got['rc']}: {got['err'][-2000:]}"
            self.dead.set()
        got["dt"] = time.time() - t0
        return got

    def run(self, script, args=(), env_extra=None, *, tag, timeout, dbg=False, route_log=None):
        """the child's JSON: the last stdout line that starts with tag"""
        import pytest   # (here, not at the top: the children import this module too)
        key = self._key(script, args, env_extra, dbg=dbg)
        if key not in self.cache and not self.dead.is_set():
            self.cache[key] = self._start(script, args, env_extra, timeout=timeout, dbg=dbg, route_log=route_log)
        if self.dead.is_set():
            pytest.exit(f"{self.dead_msg}\nnothing more is started on the GPU", returncode=3)
        got = self.cache[key]
        if "json" not in got:
            assert got["rc"] == 0, f"{script} {list(args)} {env_extra or {}} ended with status {got['rc']}: {got['err'][-3000:]}"
            got["json"] = json.loads([ln for ln in got["out"].splitlines() if ln.startswith(tag + " ")][-1][len(tag) + 1:])
            print(f"[child {script} {list(args)} {env_extra or {}} {'dbg' if dbg else 'production'}: {got['dt']:.1f} s]")
        return got["json"]

    def run_many(self, specs, workers):
        """starts the children of specs (dicts of run's arguments) that have no outcome yet, at most `workers` at a time, and records
        an outcome for every one: None for those not started because a child had died. Raises nothing: run decides."""
        todo = [s for s in specs if self._key(**s) not in self.cache]
        if todo:
            with ThreadPoolExecutor(max_workers=workers) as pool:
                for s, got in zip(todo, pool.map(lambda s: self._start(**s), todo)):
                    self.cache[self._key(**s)] = got


RUNNER = ChildRunner()


class Family:
    """one kernel family's case-matrix child (tests/kernel_pieces.py run_cases) as its parent test file sees it: the script, the tag
    of its JSON line, the route log of its debug build and its time limit, said once. Every child goes through RUNNER."""
    def __init__(self, script, tag, route_log, timeout):
        self.script, self.tag, self.route_log, self.timeout = script, tag, route_log, timeout

    def spec(self, args=(), env_extra=None, dbg=False):
        """RUNNER.run's arguments for one child (what RUNNER.run_many takes)"""
        return dict(script=self.script, args=tuple(args), env_extra=env_extra or {}, tag=self.tag, timeout=self.timeout, dbg=dbg,
                    route_log=self.route_log)

    def child(self, args=(), env_extra=None, dbg=False):
        return RUNNER.run(**self.spec(args, env_extra, dbg))

    def run(self, dtype, names=(), env_extra=None):
        """the matrix on one build: "bf16" is the debug-switch build with its route log, any other dtype the production library of
        that element type, values only"""
        if dtype == "bf16":
            return self.child(names, env_extra, True)
        return self.child(names, dict(env_extra or {}, MI355X_SD_DTYPE=dtype), False)

    @staticmethod
    def reached(got, key, declared, width):
        """the set of instantiations the cases' route lines name (key: route line -> instantiation), with a printed count of the
        cases that reach each declared one"""
        per_case = [{key(ln) for ln in v["route"]} for v in got.values()]
        for inst in declared:
            print(f"{inst:<{width}} reached by {sum(inst in c for c in per_case)} cases")
        return set().union(*per_case)

    @staticmethod
    def collect_failures(cases, got, check):
        """the messages of the AssertionErrors check(name, got[name]) raises over all cases: one failing case does not hide the rest"""
        bad = []
        for name in cases:
            try:
                check(name, got[name])
            except AssertionError as e:
                bad.append(str(e))
        return bad


# ---- child side -------------------------------------------------------------------------------------------------------------------
class Routes:
    """the lines the launchers appended to the route log that env_var names (MI355X_SD_GEMM_LOG, MI355X_SD_ATTN_LOG,
    MI355X_SD_NORM_LOG) since the last call (debug build; empty elsewhere)"""
    def __init__(self, env_var):
        self.path = os.environ.get(env_var)
        self.pos = 0

    def take(self):
        if not self.path or not os.path.exists(self.path):
            return []
        with open(self.path) as f:
            f.seek(self.pos)
            lines = f.read().splitlines()
            self.pos = f.tell()
        return lines


def emit(tag, res):
    print(tag + " " + json.dumps(res))


def sha(t):
    import torch
    t = t.contiguous().cpu()
    return hashlib.sha256(t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()).hexdigest()[:16]
