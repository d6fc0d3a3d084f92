"""Cost of the per-root diagnostics (``fk_rr_root_diagnostics``) on the device, beside the combined inference (``fk_rr_inference``) on
the same resident counts.

Two shapes:

``production``  150 strategies (11 175 pairs), two roots, blocks of 2 191 games of at most 4 382 attempts, played by
                ``fk_h2h_round_robin_resident`` with option ``"rr_keep_roots"`` on;
``synthetic``   2 000 strategies (1 999 000 pairs), two roots of binomial states (``rr_inference_cases.random_family``) through
                ``fk_rr_counts_add_root``.

Per shape and entry a warm-up and ``--reps`` (default 7) calls without rows and as many with every row: the entry's HIP events
(``fk_timing.play_ms``: the device work, copies back excluded) and the host clock around the call, min / median / max.  No threshold
is set.  Expected: without rows the diagnostics compute no interval, so they should cost less than the combined inference, whose
simultaneous interval (one per viable pair, rows or not) dominates; with rows they compute two ordinary intervals per pair (one per
root) where the inference computes one more.

    python tools/time_rr_root_diagnostics.py [--only production|synthetic] [--reps N] [--commit ID] [--out profiles/rr_root_diagnostics_timing.jsonl]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "oracle")]
KNOBS = dict(family_alpha=0.02, practical_delta=0.03, min_candidate_completion_rate=0.99)
SEEDS = (11, 12)


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def timed(eng, call, reps: int, **kwargs) -> tuple[dict, dict]:
    device, wall, result = [], [], None
    for rep in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        result = call(**KNOBS, **kwargs)
        wall.append((time.perf_counter() - t0) * 1e3)
        device.append(eng.timing()["play_ms"])
    return {"device_ms": spread(device[1:]), "wall_ms": spread(wall[1:])}, result


def main() -> None:
    import round_robin_engine_stub as stub
    import rr_inference_cases as cases
    from farkle_ii_amd.backend import Engine

    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("production", "synthetic"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rr_root_diagnostics_timing.jsonl")
    args = ap.parse_args()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with Engine(0) as eng:
        device = eng.device_info()["arch"]
        eng.rr_counts_reset()
        eng.set_option("rr_keep_roots", 1)
        for shape in ("production", "synthetic"):
            if args.only not in (None, shape):
                continue
            eng.rr_counts_reset()
            t0 = time.perf_counter()
            if shape == "production":
                n, target, cap = 150, 2191, 4382
                table = stub.random_valid_table(n, 150)
                for seed in SEEDS:
                    eng.h2h_round_robin_resident(table, seed, target, cap)
            else:
                n, target, cap = 2000, 200, 400
                table = stub.random_valid_table(n, 2000)
                for seed in SEEDS:
                    _, states, _, _ = cases.random_family(n, target, seed=seed)
                    eng.rr_counts_add(table, states[0], target, cap, root_seed=seed)
            load_s = time.perf_counter() - t0
            pairs = n * (n - 1) // 2
            line = {"what": f"rr_root_diagnostics_{shape}", "strategies": n, "pairs": pairs, "roots": len(SEEDS), "block_games": target,
                    "reps": args.reps, "load_seconds": round(load_s, 2)}
            for name, call in (("root_diagnostics", eng.rr_root_diagnostics), ("inference", eng.rr_inference)):
                line[f"{name}_no_rows"], none = timed(eng, call, args.reps)
                line[f"{name}_all_rows"], full = timed(eng, call, args.reps, rows=(0, pairs))
                if name == "root_diagnostics":
                    line["summary"] = [int(v) for v in full["summary"]]
                    if none["summary"].tolist() != line["summary"]:
                        raise SystemExit("the summary depends on the rows asked for")
                else:
                    line["class_counts"] = [int(v) for v in full["class_counts"]]
            line.update({"device": device, "commit": args.commit})
            print(json.dumps(line), flush=True)
            with args.out.open("a") as fh:
                fh.write(json.dumps(line) + "\n")
        eng.rr_counts_reset()
        eng.set_option("rr_keep_roots", 0)


if __name__ == "__main__":
    main()
