#!/usr/bin/env python3
"""Record tests/golden/power_plan_vectors.json: the reference's own power plan on the cases of tests/power_plan_cases.py.

Build container only (it imports the upstream reference through oracle/ref_import.py).  Stored, as data with floats as the hex of their
bits: ``implemented_score_test_power`` on every cell of ``golden_cells``; the SHA-256 of ``_fixed_first_count_boundary_arrays`` per
(n, alpha) of the boundary cases; ``_minimum_block_games`` with the worst-scenario power at the planned size and at the size before it
for every plan; ``_power_grid`` at the production plan.  ``measured`` holds what ``power_cells_host`` differs from the recorded powers by
(the tolerance the tests use is derived from it), the seconds the reference's scan of the production plan took and —
carried over from the existing file, where it was entered from a run on an MI355X — what the device differs from ``power_cells_host`` by.

    python tools/gen_power_plan_golden.py            # rewrite the file
    python tools/gen_power_plan_golden.py --check    # compare with the file (timings aside), exit 1 on a difference
"""
from __future__ import annotations

import argparse
import json
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "oracle")]
GOLDEN = ROOT / "tests" / "golden" / "power_plan_vectors.json"


def measured(cells, powers) -> dict:
    """The worst relative difference of ``power_cells_host`` from the recorded powers among cells whose power exceeds the absolute
    tolerance, the worst absolute difference among the others, and where the first occurs."""
    import numpy as np

    from farkle_ii_amd import h2h_power as hp

    worst_rel, worst_abs, where = 0.0, 0.0, None
    for alpha in sorted({c[3] for c in cells}):
        at = [i for i, c in enumerate(cells) if c[3] == alpha]
        got = hp.power_cells_host(hp.make_cells([cells[i][0] for i in at], [cells[i][1] for i in at], [cells[i][2] for i in at]),
                                  hp.critical_value(alpha))
        for i, g in zip(at, got):
            want = powers[i]
            if want > hp.HOST_ABS_TOL:
                rel = abs(g - want) / max(abs(g), abs(want))
                if rel > worst_rel:
                    worst_rel, where = rel, cells[i]
            else:
                worst_abs = max(worst_abs, abs(g - want))
    return {"abs_tol": hp.HOST_ABS_TOL, "worst_relative_difference": worst_rel, "rel_tol": 4.0 * worst_rel,
            "worst_case": {"n": where[0], "q_ab": where[1], "q_ba": where[2], "alpha": where[3]},
            "worst_absolute_difference_at_or_below_abs_tol": worst_abs, "cells": int(np.size(powers))}


def record() -> dict:
    import ref_import

    import power_plan_cases as cases

    ref_import.import_reference()
    from farkle.analysis import h2h_schedule as ref

    cells = cases.golden_cells()
    powers = [ref.implemented_score_test_power(*c) for c in cells]
    out = {"cells": {"count": len(cells), "power": [cases.hex_of(p) for p in powers]}, "boundaries": {}, "plans": {}}
    for alpha in cases.ALPHAS:
        for n in cases.BOUNDARY_DIGEST_NS:
            out["boundaries"][f"{n}@{cases.hex_of(alpha)}"] = cases.boundary_digest(*ref._fixed_first_count_boundary_arrays(n, alpha))
    seconds = {}
    for name in cases.PLANS:
        kw = cases.plan_settings(name)
        started = time.perf_counter()
        block = ref._minimum_block_games(**kw)
        seconds[name] = time.perf_counter() - started
        at = {k: kw[k] for k in ("root_count", "effect", "scenarios", "alpha_per_pair")}
        worst = ref._worst_scenario_power(games_per_root_order_block=block, **at)
        previous = ref._worst_scenario_power(games_per_root_order_block=block - 1, **at) if block > 1 else 0.0
        out["plans"][name] = {"block_games": int(block), "worst_scenario_achieved_power": cases.hex_of(worst),
                              "previous_equal_block_size_worst_power": cases.hex_of(previous)}
        print(f"{name}: block {block}, reference {seconds[name]:.2f} s", file=sys.stderr)
    candidates, roots, _, _, block = cases.PLANS["production"]
    cfg = types.SimpleNamespace(head2head=types.SimpleNamespace(sensitivity_deltas=(0.03, 0.04), seat1_advantage_scenarios=cases.SCENARIOS))
    grid = ref._power_grid(cfg, block_games=block, roots=tuple(range(roots)), alpha_per_pair=cases.plan_settings("production")["alpha_per_pair"])
    out["power_grid"] = [{k: (cases.hex_of(v) if isinstance(v, float) else v) for k, v in row.items()} for row in grid]
    out["measured"] = {"host_against_reference": measured(cells, powers), "reference_minimum_block_games_seconds": seconds}
    # what the device differs from power_cells_host by is measured on an MI355X (tests/test_power_plan_gpu.py prints it) and entered
    # into the file by hand, in the same form: carried over
    if GOLDEN.exists() and "device_against_host" in json.loads(GOLDEN.read_text())["measured"]:
        out["measured"]["device_against_host"] = json.loads(GOLDEN.read_text())["measured"]["device_against_host"]
    return out


def _comparable(doc: dict) -> dict:
    return {**doc, "measured": {k: v for k, v in doc["measured"].items() if k != "reference_minimum_block_games_seconds"}}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    doc = record()
    if args.check:
        same = GOLDEN.exists() and _comparable(json.loads(GOLDEN.read_text())) == _comparable(json.loads(json.dumps(doc)))
        print("golden file reproduced" if same else "golden file differs", file=sys.stderr)
        return 0 if same else 1
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    GOLDEN.write_text(text)
    print(f"wrote {GOLDEN} ({len(text)} bytes)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
