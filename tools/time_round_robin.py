"""Cost of the head-to-head round robin (``fk_h2h_round_robin``) on the device.

(a) The production family shape: 150 strategies of the default grid (evenly spaced over its 5 160), so 11 175 pairs and 22 350 blocks,
    ``target = 2 191`` and ``max_attempts = 4 382`` — beside ``fk_h2h_run_blocks`` on the identical enumerated blocks, in one process,
    warmed up, alternating, ``--reps`` (default 5) timed calls each, a host clock around the whole call (each ends in a synchronise).
    The block states of the two paths are compared for equality.  Criterion: the round-robin call is not slower than the explicit-block
    call by more than the spread (max - min) of the repeats.
(b) The full default grid: 13 310 220 pairs of 5 160 strategies, one root, ``--full-target`` completed games per block (default 8,
    ``max_attempts`` twice that) in one call: attempts per second on the host clock, the bytes returned, and the engine's own timers.
    The share of the call outside the game kernel comes from a ``rocprofv3 --kernel-trace --stats`` run of ``--only full --reps 1``.

One JSON line per part, appended to ``--out`` with the commit handed in by ``--commit``.

    python tools/time_round_robin.py [--only family|full] [--reps N] [--full-target T] [--commit ID] [--out profiles/round_robin_timing.jsonl]
"""
from __future__ import annotations

import argparse
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


def family(eng, table, reps: int) -> dict:
    from farkle_ii_amd import round_robin as rr

    n, target, max_attempts, root = 150, 2191, 4382, 42
    fam = np.ascontiguousarray(table[np.linspace(0, len(table) - 1, n).astype(np.int64)])
    pid, i, j = rr.pair_ids(n)
    seats = np.empty((2 * len(pid), 2), dtype=fam.dtype)
    seats[0::2, 0], seats[0::2, 1], seats[1::2, 0], seats[1::2, 1] = fam[i], fam[j], fam[j], fam[i]
    pids, orders = np.repeat(pid, 2), np.tile(np.arange(2), len(pid))

    def robin():
        return eng.h2h_round_robin(fam, root, target, max_attempts)[0].reshape(-1, 5)

    def explicit():
        return eng.h2h_blocks(seats, root, pids, orders, target, max_attempts, chunk_games=max_attempts).astype(np.uint32)

    a, b = robin(), explicit()  # warm-up of both paths: buffers, code objects
    if not np.array_equal(a, b):
        raise SystemExit("the round robin and the explicit-block path disagree at the family shape")
    wall = {"round_robin": [], "explicit_blocks": []}
    kernel = {"round_robin": [], "explicit_blocks": []}
    for _ in range(reps):
        for name, call in (("round_robin", robin), ("explicit_blocks", explicit)):
            t0 = time.perf_counter()
            out = call()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            kernel[name].append(eng.timing()["play_ms"])
            if not np.array_equal(out, a):
                raise SystemExit(f"{name}: states changed between repeats")
    attempts = int(a[:, 0].sum(dtype=np.int64))
    noise = max(max(v) - min(v) for v in wall.values())
    diff = statistics.median(wall["round_robin"]) - statistics.median(wall["explicit_blocks"])
    return {"what": "round_robin_family", "strategies": n, "pairs": len(pid), "blocks": 2 * len(pid), "target": target, "max_attempts": max_attempts,
            "attempts": attempts, "reps": reps, "states_equal": True,
            "wall_ms": {k: spread(v) for k, v in wall.items()}, "play_ms": {k: spread(v) for k, v in kernel.items()},
            "median_difference_ms": round(diff, 3), "spread_ms": round(noise, 3), "not_slower_within_spread": bool(diff <= noise),
            "attempts_per_s": {k: round(attempts / (statistics.median(v) * 1e-3)) for k, v in wall.items()}}


def full(eng, table, reps: int, target: int) -> dict:
    from farkle_ii_amd import round_robin as rr

    n = len(table)
    pairs = rr.pair_count(n)
    wall, play, seed, launches = [], [], [], []
    states = summary = None
    for rep in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        states, summary = eng.h2h_round_robin(table, 42, target, 2 * target)
        dt = (time.perf_counter() - t0) * 1e3
        if rep or reps == 1:
            t = eng.timing()
            wall.append(dt), play.append(t["play_ms"]), seed.append(t["seed_ms"]), launches.append(t["play_launches"])
        if reps == 1:
            break
    attempts = int(states[:, :, 0].sum(dtype=np.int64))
    if not np.array_equal(summary[:, 0], np.full(n, n - 1)) or int(summary[:, 2].sum()) != 2 * int(states[:, :, 1].sum(dtype=np.int64)):
        raise SystemExit("the full-grid summary does not add up")
    return {"what": "round_robin_full_grid", "strategies": n, "pairs": pairs, "blocks": 2 * pairs, "target": target, "max_attempts": 2 * target,
            "attempts": attempts, "completed": int(states[:, :, 1].sum(dtype=np.int64)), "reps": len(wall), "wall_ms": spread(wall),
            "play_ms": spread(play), "seed_ms": spread(seed), "play_launches": launches[-1],
            "attempts_per_s": round(attempts / (statistics.median(wall) * 1e-3)),
            "bytes_returned": int(states.nbytes + summary.nbytes), "unresolved_blocks": int((states[:, :, 1] < target).sum())}


def main() -> None:
    from farkle_ii_amd.backend import Engine
    from tools.time_config import table_for

    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("family", "full"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--full-target", type=int, default=8)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "round_robin_timing.jsonl")
    args = ap.parse_args()
    table = table_for(5160)
    with Engine(0) as eng:
        device = eng.device_info()["arch"]
        lines = []
        if args.only in (None, "family"):
            lines.append(family(eng, table, args.reps))
        if args.only in (None, "full"):
            lines.append(full(eng, table, max(1, min(args.reps, 3)), args.full_target))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with args.out.open("a") as fh:
        for line in lines:
            line = {**line, "device": device, "commit": args.commit}
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
