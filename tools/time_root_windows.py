"""Wall time of the two-root stability stage's window estimates (``fk_root_window_estimates``) at the production shape: 2 roots x
the eight production player counts, 5 160 strategies, at 100 and at 1 600 batches per cell, with the stage's real window list
(``root_stability.stage_windows``: per cell the whole matrix, the matched-count prefixes and both halves).

Per batch count one warm-up call, then ``--reps`` (at least 7) timed calls of the whole entry from the host clock (the call ends in a
stream synchronise): the host's checks of every count, upload of the 64 matrices, both kernels, download of the nine values per
window and column.  Beside it the NumPy host statement (``root_stability.estimate_windows``) on the same machine, ``--host-reps``
(at least 3) calls.  Each line goes to stdout and is appended to ``--out`` (default profiles/root_stability_windows_timing.jsonl).
Kernel-level times come from a run of this tool under ``rocprofv3 --kernel-trace --stats``.

    python tools/time_root_windows.py [--reps N] [--host-reps N] [--batches 100,1600] [--out FILE]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

S, KS = 5160, (2, 3, 4, 5, 6, 8, 10, 12)
FRACTIONS = (0.25, 0.5, 0.75, 1.0)


def inputs(batches: int, seed: int = 5) -> dict:
    rng = np.random.default_rng([seed, batches])
    exposures = [rng.integers(40, 90, size=(batches, S), dtype=np.int64) for _ in range(2) for _ in KS]
    safety = [rng.integers(0, 3, size=e.shape, dtype=np.int64) for e in exposures]
    completed = [e - f for e, f in zip(exposures, safety)]
    wins = [rng.integers(0, c // k + 1, dtype=np.int64) for k, c in zip(KS + KS, completed)]
    return {"wins": wins, "exposures": exposures, "completed": completed, "safety": safety}


def argument(name: str, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(call, reps: int) -> dict:
    seconds = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        seconds.append(time.perf_counter() - t0)
    return {"reps": reps, "call_ms_min": round(min(seconds) * 1e3, 2), "call_ms_median": round(float(np.median(seconds)) * 1e3, 2),
            "call_ms_max": round(max(seconds) * 1e3, 2)}


def main() -> None:
    from farkle_ii_amd import root_stability as rs
    from farkle_ii_amd.engine import get_engine

    reps, host_reps = max(argument("--reps", 7), 7), max(argument("--host-reps", 3), 3)
    out = Path(argument("--out", str(ROOT / "profiles" / "root_stability_windows_timing.jsonl")))
    eng = get_engine()
    info = eng.device_info()
    out.parent.mkdir(parents=True, exist_ok=True)
    for batches in [int(b) for b in argument("--batches", "100,1600").split(",")]:
        mats = inputs(batches)
        windows, _ = rs.stage_windows([batches] * (2 * len(KS)), S, rs.DEFAULT_STAGE_BATCH_BYTES, FRACTIONS)
        shape = {"strategies": S, "roots": 2, "player_counts": len(KS), "batches_per_cell": batches, "windows": len(windows),
                 "window_rows": int((windows[:, 2] - windows[:, 1]).sum()), "pairwise_windows": int(np.count_nonzero(windows[:, 3] < S)),
                 "matrix_bytes": int(sum(m.nbytes for group in mats.values() for m in group))}
        device = eng.root_window_estimates(**mats, windows=windows)  # warm-up: code objects, buffers
        lines = [{"what": "fk_root_window_estimates, whole entry from the host clock", **shape, "device": info["arch"],
                  **timed(lambda: eng.root_window_estimates(**mats, windows=windows), reps)}]
        host = rs.estimate_windows(**mats, windows=windows)
        same = all(np.ascontiguousarray(device[name]).tobytes() == np.ascontiguousarray(host[name]).tobytes() for name in host)
        lines.append({"what": "root_stability.estimate_windows (NumPy host statement), same machine", **shape, "equal_to_the_device_bit_for_bit": same,
                      **timed(lambda: rs.estimate_windows(**mats, windows=windows), host_reps)})
        with open(out, "a") as sink:
            for line in lines:
                print(json.dumps(line), flush=True)
                sink.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
