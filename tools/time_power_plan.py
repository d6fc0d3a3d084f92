"""Cost of the round robin's power plan (``fk_score_power_scan``, ``farkle round-robin --plan-power --plan-only``) at the production
settings: 150 candidates, 2 roots, ``family_alpha`` 0.02, effect 0.03, scenarios (0, 0.03, 0.06), target power 0.80.

Three things, a warm-up and ``--reps`` (default 5) repetitions each, min / median / max:

``scan``      the production scan as the plan issues it — block sizes 1 .. 2304 in windows of 256, three cells per size — the entry's
              HIP events (``fk_timing.play_ms``) summed over the nine calls, the host clock around them, and the same cells as one call;
``plan``      ``h2h_power.plan_block_games`` on the engine: the scan, the host statement's evaluations that decide it, the curve;
``command``   ``farkle round-robin --plan-power --plan-only`` in this process from argument list to the two files: configuration,
              strategy grid, plan, document, ``power_validation``, both writes.

``--reference`` (build container only: it imports the upstream reference through oracle/ref_import.py) times the reference's own
``_minimum_block_games`` at the same settings on the CPU and writes ``profiles/power_plan_reference_cpu.json``; a later device run
copies that figure beside its own, for context only.  No threshold is set.

    python tools/time_power_plan.py [--reps N] [--commit ID] [--out profiles/power_plan_timing.jsonl]
    python tools/time_power_plan.py --reference
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "oracle")]
REFERENCE_FILE = ROOT / "profiles" / "power_plan_reference_cpu.json"
SETTINGS = dict(root_count=2, effect=0.03, scenarios=(0.0, 0.03, 0.06), alpha_per_pair=0.02 / 11175, target_power=0.80)
CANDIDATES = 150


def spread(values) -> dict:
    return {"min": round(min(values), 4), "median": round(statistics.median(values), 4), "max": round(max(values), 4)}


def time_reference(reps: int) -> None:
    import ref_import

    ref_import.import_reference()
    from farkle.analysis import h2h_schedule as ref

    seconds, block = [], None
    for _ in range(reps):
        ref.implemented_score_test_power.cache_clear()
        started = time.perf_counter()
        block = ref._minimum_block_games(**SETTINGS)
        seconds.append(time.perf_counter() - started)
    doc = {"what": "the reference's _minimum_block_games at the production settings, CPU", "block_games": int(block), "seconds": spread(seconds)}
    REFERENCE_FILE.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


def time_device(reps: int, commit: str | None, out: Path) -> None:
    from farkle_ii_amd import h2h_power as hp
    from farkle_ii_amd.backend import Engine
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.engine import set_engine

    q = np.array([hp.scenario_probabilities(SETTINGS["effect"], s) for s in SETTINGS["scenarios"]])
    windows = []
    for first in range(1, 2305, hp.DEFAULT_WINDOW):
        blocks = np.arange(first, first + hp.DEFAULT_WINDOW)
        windows.append(hp.make_cells(np.repeat(blocks * 2, 3), np.tile(q[:, 0], len(blocks)), np.tile(q[:, 1], len(blocks))))
    whole = np.concatenate(windows)
    rows = []
    with Engine(0) as eng, tempfile.TemporaryDirectory() as tmp:
        device, wall, one_device, one_wall, plan_wall, command_wall = [], [], [], [], [], []
        plan = None
        for rep in range(reps + 1):
            started, ms = time.perf_counter(), 0.0
            for cells in windows:
                eng.score_power_scan(cells, SETTINGS["alpha_per_pair"])
                ms += eng.timing()["play_ms"]
            elapsed = time.perf_counter() - started
            started = time.perf_counter()
            eng.score_power_scan(whole, SETTINGS["alpha_per_pair"])
            elapsed_one, ms_one = time.perf_counter() - started, eng.timing()["play_ms"]
            hp.score_test_power.cache_clear()
            started = time.perf_counter()
            plan = hp.plan_block_games(eng, **SETTINGS)
            elapsed_plan = time.perf_counter() - started
            if rep:  # (the first repetition warms up)
                device.append(ms), wall.append(1e3 * elapsed), one_device.append(ms_one), one_wall.append(1e3 * elapsed_one), plan_wall.append(1e3 * elapsed_plan)
        # the command: the first 150 strategies of the default grid are the family
        from farkle_ii_amd import runner
        from farkle_ii_amd.config import AppConfig

        grid, _ = runner._resolve_strategies(AppConfig(), None)
        ids_file = Path(tmp) / "family.txt"
        ids_file.write_text("".join(f"{i}\n" for i in sorted(int(s.strategy_id) for s in grid)[:CANDIDATES]))
        set_engine(eng)
        try:
            for rep in range(reps + 1):
                hp.score_test_power.cache_clear()
                started = time.perf_counter()
                main(["--set", f"io.results_dir_prefix={tmp}/out", "--set", "sim.seed_list=[11, 12]", "--log-level", "WARNING", "round-robin", "--plan-power", "--plan-only",
                      "--strategy-ids", str(ids_file), "--out", str(Path(tmp) / f"plan{rep}")])
                if rep:
                    command_wall.append(1e3 * (time.perf_counter() - started))
            doc = json.loads((Path(tmp) / "plan1" / "h2h_power_plan.json").read_text())
        finally:
            set_engine(None)
        info = eng.device_info()
    row = {"what": "power plan, production settings", "commit": commit, "device": info["name"], "reps": reps, "block_games": plan["block_games"],
           "command_block_games": doc["n_completed_required_per_root_order_block"], "host_evaluations": plan["host_evaluations"],
           "cells": int(len(whole)), "scan_windows": len(windows), "scan_device_ms": spread(device), "scan_wall_ms": spread(wall),
           "scan_one_call_device_ms": spread(one_device), "scan_one_call_wall_ms": spread(one_wall), "plan_wall_ms": spread(plan_wall),
           "command_plan_only_wall_ms": spread(command_wall)}
    if REFERENCE_FILE.exists():
        row["reference_minimum_block_games_cpu_seconds"] = json.loads(REFERENCE_FILE.read_text())["seconds"]
    rows.append(row)
    with out.open("a") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


def main_() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "power_plan_timing.jsonl")
    ap.add_argument("--reference", action="store_true", help="time the reference's scan on the CPU instead (build container only)")
    args = ap.parse_args()
    if args.reference:
        time_reference(max(1, min(args.reps, 3)))  # (ten seconds a repetition)
    else:
        time_device(args.reps, args.commit, args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main_())
