"""Cost of the seat-analysis stage on the device (``fk_tournament_run_seat_counts``: the per-seat counts gather and, at k = 2, the
mirrored-pair sort-and-segment reduce) beyond its game kernel, at the shapes of bench configs 2 and 3, next to the same figure
of the all-seat statistics pass (``fk_tournament_run_stats``) on the same range in the same process.

Per shape: one warm-up call and seven timed calls of each variant, from the engine's HIP events (``Engine.timing``): ``beyond_ms`` =
total_ms - play_ms (everything of the call on the device that is not the game kernel), reported as min / median / max.  Variants:
``plain`` (fk_tournament_run: what every call pays), ``seat_counts``, ``seat_counts_pairs`` (k = 2 only) and ``seat_stats``.
Kernel-level times (sort, segment, pair sum) come from a run of this tool under ``rocprofv3 --kernel-trace --stats``.

    python tools/time_seat_analysis.py [config2|config3|all] [--reps N] [--out profiles/seat_analysis_timing.jsonl]
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def shapes(which: str):
    from bench import grid64
    from tools.time_config import table_for

    out = []
    if which in ("config2", "all"):
        out.append(("config2", grid64(), 2, 42, 312_500))
    if which in ("config3", "all"):
        out.append(("config3", table_for(5160), 4, 0, 77_520))
    return out


def main() -> None:
    from farkle_ii_amd.engine import get_engine

    which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "all"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    info = eng.device_info()
    lines = []
    for label, table, k, root, n_sh in shapes(which):
        ids = np.asarray(table["strategy_id"], dtype=np.int32)
        if len(np.unique(ids)) != len(ids):
            ids = np.arange(len(table), dtype=np.int32)
        variants = {"plain": lambda: eng.tournament(table, k, root, 0, n_sh),
                    "seat_counts": lambda: eng.tournament_seat_counts(table, k, root, 0, n_sh),
                    "seat_stats": lambda: eng.tournament(table, k, root, 0, n_sh, want_seat_stats=True, want_seat_ratios=False)}
        if k == 2:
            variants["seat_counts_pairs"] = lambda: eng.tournament_seat_counts(table, k, root, 0, n_sh, strategy_ids=ids, want_mirrored=True,
                                                                               pair_capacity=len(table) * (len(table) - 1) // 2)
        line = {"shape": label, "k": k, "strategies": len(table), "shuffles": n_sh, "games": n_sh * (len(table) // k),
                "device": info["arch"], "reps": reps}
        for name, call in variants.items():
            call()  # warm-up: buffers, hipcub scratch
            beyond, play = [], []
            for _ in range(reps):
                call()
                t = eng.timing()
                beyond.append(t["total_ms"] - t["play_ms"])
                play.append(t["play_ms"])
            line[name] = {"beyond_ms": {"min": round(min(beyond), 3), "median": round(statistics.median(beyond), 3), "max": round(max(beyond), 3)},
                          "play_ms_median": round(statistics.median(play), 3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
