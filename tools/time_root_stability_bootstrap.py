"""Wall time of the two-root stability stage's bootstrap families on the device (``fk_root_stability_bootstrap``) at the production
shape: 2 roots x the eight production player counts x 100 batches, 5 160 strategies, 2 000 replicates.

One warm-up call, then ``--reps`` (at least 7) timed calls of the whole entry from the host clock (the call ends in a stream
synchronise): upload of the sixteen matrices, draws, the rates pass, two rank passes, download — both families as ``farkle
root-stability`` calls it ("both"), the top-N family alone ("top_n") and with the per-replicate membership of the top-N range writer
("both+membership").  Kernel-level times come from a run of this tool under ``rocprofv3 --kernel-trace --stats``.  The comparison
figure is the reference's own two range writers + reductions on the CPU: ``tools/gen_root_stability_golden.py --time``.

    python tools/time_root_stability_bootstrap.py [--reps N] [--out FILE]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

S, KS, BATCHES, REPLICATES = 5160, (2, 3, 4, 5, 6, 8, 10, 12), 100, 2000


def inputs(seed: int = 5):
    rng = np.random.default_rng(seed)
    exposures = [rng.integers(40, 90, size=(BATCHES, S), dtype=np.int64) for _ in range(2) for _ in KS]
    wins = [rng.integers(0, e // k + 1, dtype=np.int64) for k, e in zip(KS + KS, exposures)]
    joint = {"observed": rng.normal(0.0, 0.02, size=(len(KS), S)), "expected": rng.uniform(0.005, 0.05, size=(len(KS), S)),
             "observed_across": rng.normal(0.0, 0.01, size=S), "expected_across": rng.uniform(0.002, 0.02, size=S)}
    return wins, exposures, joint


def main() -> None:
    from farkle_ii_amd.engine import get_engine

    reps = max(int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7, 7)
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    info = eng.device_info()
    wins, exposures, joint = inputs()
    weights = [1.0 / len(KS)] * len(KS)
    lines = []
    for variant, kw in (("both", joint), ("top_n", {}), ("both+membership", dict(joint, want_membership=True))):
        call = lambda: eng.root_stability_bootstrap((7, 19), KS, wins, exposures, weights, 0, REPLICATES, 75, **kw)  # noqa: E731
        call()  # warm-up: code objects, buffers
        seconds = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            seconds.append(time.perf_counter() - t0)
        line = {"what": "fk_root_stability_bootstrap, whole entry from the host clock", "variant": variant, "strategies": S, "roots": 2,
                "player_counts": len(KS), "batches": 2 * len(KS) * BATCHES, "replicates": REPLICATES,
                "multiply_adds": 2 * S * 2 * len(KS) * BATCHES * REPLICATES, "device": info["arch"], "reps": reps,
                "call_ms_min": round(min(seconds) * 1e3, 2), "call_ms_median": round(float(np.median(seconds)) * 1e3, 2),
                "call_ms_max": round(max(seconds) * 1e3, 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
