"""Cost of the roll census (``fk_census_games`` / ``fk_tournament_run_census``) on the device.

(a) ``census_games`` on the 10 000-game two-seat list of tools/time_trace.py (the 64-strategy grid of bench config 2, namespace-103
    coordinates, default target and round limit), beside ``fk_trace_games``' COUNTING call (``events = NULL``: the counting pass and
    its rows, no event stored) on the same list.  Both play the same game loop from the same table-free device functions; the ratio
    of the two kernel times is reported.
(b) ``tournament_census`` of one production deterministic batch — the workload planner's ``shuffles_per_batch`` for the default
    configuration — of the 5 160-strategy grid at two and at five seats, in games per second.

One warm-up and ``--reps`` (default 7) timed calls each; kernel times from the engine's HIP events (``Engine.timing``: ``play_ms``), the
whole call on the host clock beside them.  Reported as min / median / max; appended to ``--out``.

    python tools/time_census.py [--reps N] [--out profiles/census_timing.jsonl]
"""
from __future__ import annotations

import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def counting_trace(eng, coords, table, ss, k) -> int:
    """``fk_trace_games`` with ``events = NULL``: rows and event_begin only; returns the rolls of the list."""
    from farkle_ii_amd.backend import COORD_DTYPE, STRATEGY_DTYPE, _p, row_dtype

    coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
    table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE)
    ss = np.ascontiguousarray(ss, dtype=np.int32).reshape(-1)
    rows, begin = np.zeros(len(coords), dtype=row_dtype(k)), np.zeros(len(coords) + 1, dtype=np.int64)
    eng._check(eng._lib.fk_trace_games(eng._ctx, _p(coords), C.c_int64(len(coords)), _p(table), C.c_int32(len(table)), _p(ss), C.c_int32(k),
                                       C.c_int32(10_000), C.c_int32(200), _p(rows), _p(begin), None, C.c_int64(0)))
    return int(begin[-1])


def timed(reps: int, call, eng):
    call()  # warm-up: buffers
    kernel_ms, wall_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(eng.timing()["play_ms"])
    return kernel_ms, wall_ms


def main() -> None:
    from bench import grid64
    from farkle_ii_amd import runner
    from farkle_ii_amd.backend import make_coords
    from farkle_ii_amd.config import AppConfig
    from farkle_ii_amd.engine import get_engine
    from tools.time_config import table_for

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    arch = eng.device_info()["arch"]
    lines = []

    n = 10_000
    table = grid64()
    rs = np.random.default_rng(n)
    coords = make_coords(103, 42, 2, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 32, size=n))
    ss = rs.integers(0, len(table), size=(n, 2))
    rolls = counting_trace(eng, coords, table, ss, 2)
    census = eng.census_games(coords, table, ss, 2)
    assert int(census["roll_cells"].sum()) == rolls
    census_ms, census_wall = timed(reps, lambda: eng.census_games(coords, table, ss, 2), eng)
    trace_ms, trace_wall = timed(reps, lambda: counting_trace(eng, coords, table, ss, 2), eng)
    line = {"what": "census_games", "games": n, "k": 2, "strategies": len(table), "rolls": rolls, "device": arch, "reps": reps,
            "census": {"play_ms": spread(census_ms), "wall_ms": spread(census_wall)},
            "trace_counting_call": {"play_ms": spread(trace_ms), "wall_ms": spread(trace_wall)},
            "census_over_trace_counting": round(statistics.median(census_ms) / statistics.median(trace_ms), 3)}
    lines.append(line)
    print(json.dumps(line), flush=True)

    big = table_for(5160)
    for k in (2, 5):
        n_sh = int(runner._plan_workload_from_config(AppConfig(), len(big), k).shuffles_per_batch)
        games = n_sh * (len(big) // k)
        holder = {}

        def call(k=k, n_sh=n_sh):
            holder["census"] = eng.tournament_census(big, k, 0, 0, n_sh)

        kernel_ms, wall_ms = timed(reps, call, eng)
        eng.tournament(big, k, 0, 0, n_sh)
        hot_ms = eng.timing()["play_ms"]
        line = {"what": "tournament_census", "games": games, "k": k, "strategies": len(big), "shuffles": n_sh,
                "rolls": int(holder["census"]["roll_cells"].sum()), "device": arch, "reps": reps, "play_ms": spread(kernel_ms),
                "wall_ms": spread(wall_ms), "games_per_s": round(games / (statistics.median(wall_ms) * 1e-3)),
                "kernel_games_per_s": round(games / (statistics.median(kernel_ms) * 1e-3)), "game_kernel_play_ms_same_range": round(hot_ms, 3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
