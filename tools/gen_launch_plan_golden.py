"""TEST INFRASTRUCTURE ONLY — write tests/golden/launch_plan.json: the game kernel's launch plan for every call of
tests/launch_plan_cases.py: inputs(), as the host program tests/native/launch_plan_host_check.hip prints it.  No GPU, no oracle.

The committed fixture was written from the planner of commit f7fefeb (plan_play, plan_play_hc and play_lds_bytes of farkle_hip.hip moved
into a header verbatim, the five fk_ctx fields no option could set as constants at their defaults, the shape named by a transcription of
that commit's launch_play ladders), BEFORE the planner became a walk over the instance table: it pins the refactor and is not rewritten
from the refactored code.  Run this again only when a plan is meant to change (a new shape, a new option), and review the diff of the
fixture line by line; a program for another source state's planner (same input and output lines) can be given as the argument.

    python tools/gen_launch_plan_golden.py [planner_program.hip]
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tests"))
import launch_plan_cases as lp  # noqa: E402


def main() -> None:
    source = Path(sys.argv[1]) if len(sys.argv) > 1 else lp.SOURCE
    cases = lp.inputs()
    with tempfile.TemporaryDirectory() as tmp:
        plans = lp.run_planner(lp.build_planner(Path(tmp), source), cases)
    lp.check_conditions(cases, plans)
    # every distinct plan once (None: no instance), the calls refer to it by number in the order of inputs()
    distinct: dict[tuple | None, int] = {}
    index = [distinct.setdefault(None if p is None else tuple(p[f] for f in lp.PLAN_FIELDS), len(distinct)) for p in plans]
    rows = ",\n".join(json.dumps(list(p) if p is not None else None, separators=(",", ":")) for p in distinct)
    calls = ",\n".join(",".join(str(i) for i in index[at:at + 36]) for at in range(0, len(index), 36))
    lp.FIXTURE.write_text('{"fields":%s,\n"calls":%d,\n"plans":[\n%s],\n"plan_of_call":[\n%s]}\n'
                          % (json.dumps(list(lp.PLAN_FIELDS), separators=(",", ":")), len(cases), rows, calls))
    assert json.loads(lp.FIXTURE.read_text())["plan_of_call"] == index
    none = sum(p is None for p in plans)
    print(lp.FIXTURE, lp.FIXTURE.stat().st_size, "bytes;", len(cases), "calls,", len(distinct), "distinct plans,", none, "without an instance")
    assert lp.FIXTURE.stat().st_size < 256 * 1024


if __name__ == "__main__":
    main()
