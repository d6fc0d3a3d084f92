"""Cost of the roll-level trace (``fk_trace_games``) next to ``fk_play_games`` on the same game list: 200 and 10 000 two-seat games of
the 64-strategy grid of bench config 2, namespace-103 coordinates, default target and round limit.

Per list: one warm-up and ``--reps`` timed calls of each, from the engine's HIP events (``Engine.timing``).  ``trace`` is the
exact-size call ``Engine.trace_games`` ends with — ``play_ms`` = its counting pass + its writing pass — and ``trace_wall_ms`` the
whole ``Engine.trace_games`` (the counting call in front of it, both scans, every copy) on the host clock; ``play`` is
``fk_play_games``' game kernel (``play_ms``) and seeding (``seed_ms``).  Reported as min / median / max.

    python tools/time_trace.py [--reps N] [--out profiles/trace_timing.jsonl]
"""
from __future__ import annotations

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


def main() -> None:
    from bench import grid64
    from farkle_ii_amd.backend import make_coords
    from farkle_ii_amd.engine import get_engine

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    table = grid64()
    lines = []
    for n in (200, 10_000):
        rs = np.random.default_rng(n)
        coords = make_coords(103, 42, 2, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 32, size=n))
        ss = rs.integers(0, len(table), size=(n, 2))
        rows, begin, events = eng.trace_games(coords, table, ss, 2)  # warm-up: buffers, hipcub scratch
        assert rows.tobytes() == eng.play_games(coords, table, ss, 2).tobytes()
        trace_ms, wall_ms, play_ms, seed_ms = [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.trace_games(coords, table, ss, 2)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            trace_ms.append(eng.timing()["play_ms"])
            eng.play_games(coords, table, ss, 2)
            t = eng.timing()
            play_ms.append(t["play_ms"])
            seed_ms.append(t["seed_ms"])
        line = {"games": n, "k": 2, "events": int(begin[-1]), "longest_game": int(np.diff(begin).max()), "device": eng.device_info()["arch"],
                "reps": reps, "trace": {"play_ms": spread(trace_ms)}, "trace_wall_ms": spread(wall_ms),
                "play": {"play_ms": spread(play_ms), "seed_ms": spread(seed_ms)}}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
