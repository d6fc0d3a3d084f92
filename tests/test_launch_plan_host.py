"""CPU check of the game kernel's launch planner: csrc/fk_plan.h is plain host C++, so tests/native/launch_plan_host_check.hip plans every
call of tests/launch_plan_cases.py: inputs() without a GPU, and every plan must equal the one tests/golden/launch_plan.json records for
that call, field for field: block, grid, LDS bytes, LDS tally, record layout, kernel, and which of the 21 shapes it names (or that no
instance fits).  The fixture was written from the planner as it stood before it became a walk over the instance table
(tools/gen_launch_plan_golden.py), so a refactor of the planner that changes any plan fails here.  No GPU, no oracle."""
from __future__ import annotations

import json
import shutil
from pathlib import Path

import pytest

import launch_plan_cases as lp


@pytest.mark.skipif(not (shutil.which(lp.HIPCC) or Path(lp.HIPCC).exists()), reason="hipcc not available")
def test_every_plan_equals_its_fixture_line(tmp_path):
    fixture = json.loads(lp.FIXTURE.read_text())
    assert lp.FIXTURE.stat().st_size < 256 * 1024 and tuple(fixture["fields"]) == lp.PLAN_FIELDS
    cases = lp.inputs()
    assert fixture["calls"] == len(cases) == len(fixture["plan_of_call"])
    want = [None if row is None else dict(zip(lp.PLAN_FIELDS, row)) for row in fixture["plans"]]
    want = [want[i] for i in fixture["plan_of_call"]]
    lp.check_conditions(cases, want)  # all 21 shapes, a call without an instance, at most 10 % of them
    got = lp.run_planner(lp.build_planner(tmp_path), cases)
    wrong = []
    for case, g, w in zip(cases, got, want):
        if g != w:
            fields = "instance / none" if g is None or w is None else ", ".join(f"{f}: {g[f]} != {w[f]}" for f in lp.PLAN_FIELDS if g[f] != w[f])
            wrong.append(f"{case}: {fields}")
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ from tests/golden/launch_plan.json:\n" + "\n".join(wrong[:40])
