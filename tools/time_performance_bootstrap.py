"""Wall time of the joint batch bootstrap on the device (``fk_performance_bootstrap``) at the production shape (5 160 strategies, the
eight production player counts x 100 batches, 2 000 replicates) and at one large shape (one player count, 1 800 batches).

Per shape: one warm-up call, then ``--reps`` timed calls of the whole entry from the host clock (the call ends in a stream
synchronise): upload of the matrices, draws, integer product, ranks, contrasts, download of the sums — without the replicate scores,
as ``farkle run --performance-bootstrap`` calls it — and once with them (the range writer's payload).  Kernel-level times come from a run of this tool under
``rocprofv3 --kernel-trace --stats``.  The comparison figure is the reference's own range writer + reduction on the CPU:
``tools/gen_performance_bootstrap_golden.py --time``.

    python tools/time_performance_bootstrap.py [production|large|all] [--reps N] [--out profiles/performance_bootstrap_timing.jsonl]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"production": (5160, {k: 100 for k in (2, 3, 4, 5, 6, 8, 10, 12)}, 2000), "large": (5160, {4: 1800}, 2000)}


def matrices(S: int, batches: dict, seed: int = 5):
    rng = np.random.default_rng(seed)
    ks = sorted(batches)
    exposures = [rng.integers(40, 90, size=(batches[k], S), dtype=np.int64) for k in ks]
    wins = [rng.integers(0, e // k + 1, dtype=np.int64) for k, e in zip(ks, exposures)]
    return ks, wins, exposures


def main() -> None:
    from farkle_ii_amd.engine import get_engine

    which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "all"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    info = eng.device_info()
    lines = []
    for label in (SHAPES if which == "all" else [which]):
        S, batches, replicates = SHAPES[label]
        ks, wins, exposures = matrices(S, batches)
        for variant, want_scores in (("sums", False), ("sums+scores", True)):
            call = lambda: eng.performance_bootstrap(7, ks, wins, exposures, 0, replicates, 75, 0.03, controls=[0, 17],  # noqa: E731
                                                     want_scores=want_scores)
            call()  # warm-up: code objects, buffers
            seconds = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                seconds.append(time.perf_counter() - t0)
            line = {"shape": label, "variant": variant, "strategies": S, "player_counts": len(ks), "batches": sum(batches.values()),
                    "replicates": replicates, "multiply_adds": 2 * S * sum(batches.values()) * replicates, "device": info["arch"],
                    "reps": reps, "call_ms_min": round(min(seconds) * 1e3, 2), "call_ms_median": round(float(np.median(seconds)) * 1e3, 2),
                    "call_ms_max": round(max(seconds) * 1e3, 2)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
