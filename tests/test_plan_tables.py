"""CPU: every planner's launch plan, rebuilt on the host-memory emulator, is the one recorded in tests/golden/plan_tables.json
before the planners moved onto paddlemix_amd.program.PlanBuilder -- launch for launch (entry point, kind string, flops) and, through
the digest of the exported program's tables, argument for argument with every pointer as (region, byte offset) and the regions in
allocation order. Cases and recorder: tests/plan_table_cases.py."""
import json
import os

import pytest

from tests import plan_table_cases as PT

GOLDEN = {}
for _name in ("plan_tables.json", "plan_tables_later.json"):   # (the cases of models that came after the first recording)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", _name)) as _fh:
        _cases = json.load(_fh)["cases"]
    assert not set(_cases) & set(GOLDEN), _name
    GOLDEN.update(_cases)


def test_fixture_and_cases_name_the_same_plans():
    assert sorted(GOLDEN) == sorted(PT.CASES)


@pytest.mark.parametrize("name", list(PT.CASES))
def test_plan_is_the_recorded_one(name):
    got, want = PT.record(name), GOLDEN[name]
    assert len(got) == len(want), f"{name}: {len(got)} cached plans, {len(want)} recorded"
    for i, (g, w) in enumerate(zip(got, want)):
        where = f"{name}, plan {i}"
        for n, (a, b) in enumerate(zip(g["prog"], w["prog"])):
            assert a == b, f"{where}: launch {n} is {a[0]} [{a[1]}, {a[2]:g} flop], recorded {b[0]} [{b[1]}, {b[2]:g} flop]"
        m, longer = min(g["launches"], w["launches"]), (g if g["launches"] > w["launches"] else w)
        assert g["launches"] == w["launches"], (
            f"{where}: {g['launches']} launches, {w['launches']} recorded; the first {m} agree, then launch {m} "
            f"({longer['prog'][m][0]}) is {'extra' if longer is g else 'missing'}")
        assert g["tables_sha256"] == w["tables_sha256"], (
            f"{where}: all {w['launches']} launches agree in entry point, kind and flops, but the exported tables differ "
            "(an argument value, a scratch buffer's size or sharing, or the order buffers are allocated in)")
