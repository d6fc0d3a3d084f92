"""Cost of the round-robin inference (``fk_rr_inference``) on the device, and what keeping the states resident is worth.

(a) The production family shape: 150 strategies of the default grid (evenly spaced over its 5 160), 11 175 pairs, ``target = 2 191``,
    ``max_attempts = 4 382``, one root.
(b) The full default grid: 13 310 220 pairs of 5 160 strategies, one root, ``--full-target`` completed games per block (default 8).

Per shape: the resident round-robin call beside ``fk_h2h_round_robin`` on the same range (host clock around each call, which ends in
a synchronise; alternating, after a warm-up); then ``fk_rr_inference`` with ``rows`` null and with a row slice (every pair of the
family, 2^20 rows of the full grid), a warm-up and ``--reps`` (default 7) calls each: the entry's own HIP events around its device work
(``fk_timing.play_ms``) and the host clock around the call, min / median / max.  For scale, the host statement
(``rr_inference.infer``, the plain loop) on the first 1 000 pairs of the same counts.  No threshold is set.

One JSON line per shape, appended to ``--out`` with the commit handed in by ``--commit``.

    python tools/time_rr_inference.py [--only family|full] [--reps N] [--full-target T] [--commit ID] [--out profiles/rr_inference_timing.jsonl]
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

KNOBS = dict(family_alpha=0.02, practical_delta=0.03, delta_equivalence=None, min_candidate_completion_rate=0.99)


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def shape(eng, what: str, table, target: int, max_attempts: int, reps: int, slice_rows: int) -> dict:
    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd import rr_inference as ri

    n, root = len(table), 42
    pairs = rr.pair_count(n)

    def plain():
        return eng.h2h_round_robin(table, root, target, max_attempts)

    def resident():
        eng.rr_counts_reset()
        return eng.h2h_round_robin_resident(table, root, target, max_attempts)

    states, summary = plain()  # warm-up of both paths: buffers, code objects
    if not np.array_equal(resident(), summary):
        raise SystemExit(f"{what}: the resident round robin's summary differs")
    wall = {"round_robin": [], "round_robin_resident": []}
    for _ in range(min(reps, 3)):
        for name, call in (("round_robin", plain), ("round_robin_resident", resident)):
            t0 = time.perf_counter()
            call()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    # the accumulator now holds the last resident call's root
    out = {"what": what, "strategies": n, "pairs": pairs, "target": target, "max_attempts": max_attempts, "reps": reps,
           "round_robin_wall_ms": {k: spread(v) for k, v in wall.items()}, "states_bytes_kept_on_device": int(states.nbytes)}
    class_counts = None
    for name, rows in (("rows_null", None), (f"rows_{slice_rows}", (0, slice_rows))):
        device_ms, wall_ms = [], []
        for rep in range(reps + 1):  # the first call warms up
            t0 = time.perf_counter()
            result = eng.rr_inference(rows=rows, **KNOBS)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                device_ms.append(eng.timing()["play_ms"]), wall_ms.append(dt)
        if class_counts is not None and not np.array_equal(class_counts, result["class_counts"]):
            raise SystemExit(f"{what}: class counts changed between calls")
        class_counts = result["class_counts"]
        out[name] = {"device_ms": spread(device_ms), "wall_ms": spread(wall_ms)}
    out["class_counts"] = {k: int(v) for k, v in zip(ri.DECISION_CLASSES, class_counts)}
    out["pairs_per_s_rows_null"] = round(pairs / (out["rows_null"]["device_ms"]["median"] * 1e-3))
    # the host statement on 1 000 pairs of the same counts, the plain loop
    head = min(1000, pairs)
    counts = ri.combine_counts([states[:head]], [target], [max_attempts])
    t0 = time.perf_counter()
    ri.infer(n, counts, family_pair_count=pairs, **KNOBS)
    out["host_statement_1000_pairs_ms"] = round((time.perf_counter() - t0) * 1e3 * (1000 / head), 1)
    eng.rr_counts_reset()
    return out


def main() -> None:
    from farkle_ii_amd.backend import Engine
    from tools.time_config import table_for

    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("family", "full"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--full-target", type=int, default=8)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rr_inference_timing.jsonl")
    args = ap.parse_args()
    table = table_for(5160)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with Engine(0) as eng:
        device = eng.device_info()["arch"]
        todo = []
        if args.only in (None, "family"):
            fam = np.ascontiguousarray(table[np.linspace(0, len(table) - 1, 150).astype(np.int64)])
            todo.append(("rr_inference_family", fam, 2191, 4382, 11_175))
        if args.only in (None, "full"):
            todo.append(("rr_inference_full_grid", table, args.full_target, 2 * args.full_target, 1 << 20))
        for what, tab, target, cap, slice_rows in todo:
            line = {**shape(eng, what, tab, target, cap, args.reps, slice_rows), "device": device, "commit": args.commit}
            print(json.dumps(line), flush=True)
            with args.out.open("a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
