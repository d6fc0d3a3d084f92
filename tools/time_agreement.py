"""Cost of the method agreement on the device: ``fk_rr_agreement`` beyond ``fk_rr_inference``, and ``fk_rank_concordance`` alone.

Two table sizes — 150 strategies (the reference's finalists, 11 175 pairs) and 5 160 (the whole default grid, 13 310 220 pairs) —
each with a scored population of 5 160.  The resident counts are one root of seeded binomial block states (``rr_counts_add``); the
ranks are a seeded permutation and a noisy copy of it with ties, a few of them null.

Per shape a warm-up and ``--reps`` (default 5) calls: ``fk_rr_inference`` without rows (``fk_timing``: ``play_ms``), ``fk_rr_agreement``
with the codes null (``play_ms`` the whole chain, ``perm_ms`` the pair pass in it) and with the codes, and ``fk_rank_concordance``
(``play_ms``), each with the host clock around the call; min / median / max.  No threshold is set.  The reference's
``_pair_agreement`` seconds on the 150-strategy golden case are copied from tests/golden/agreement_vectors.json, for context only.

    python tools/time_agreement.py [--only 150|5160] [--reps N] [--commit ID] [--out profiles/agreement_timing.jsonl]
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
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
GOLDEN = ROOT / "tests" / "golden" / "agreement_vectors.json"
GAMES, POPULATION = 200, 5160
PARAMS = dict(family_alpha=0.02, practical_delta=0.03, delta_equivalence=0.03, min_candidate_completion_rate=0.99)


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def states(n: int, seed: int = 23) -> np.ndarray:
    """One root's block states uint32 ``[pairs, 2, 5]``: every block reaches its target, rates spread around one half."""
    from farkle_ii_amd import round_robin as rr

    rng = np.random.default_rng(seed + n)
    _, i, j = rr.pair_ids(n)
    skill = rng.normal(0.0, 0.08, size=n)
    gap = np.clip(skill[i] - skill[j], -0.45, 0.45)
    st = np.zeros((len(i), 2, 5), dtype=np.uint32)
    st[:, :, 0] = st[:, :, 1] = GAMES
    st[:, 0, 3], st[:, 1, 3] = rng.binomial(GAMES, 0.5 + gap), rng.binomial(GAMES, 0.5 - gap)
    st[:, :, 4] = GAMES - st[:, :, 3]
    return st


def ranks(m: int, seed: int = 29) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(seed + m)
    win = (1 + rng.permutation(m)).astype(np.int32)
    ts = (1 + (win + rng.normal(0.0, m / 6.0, size=m)).argsort().argsort() // 2).astype(np.int32)  # ties in pairs
    return win, ts


def timed(call, eng, reps: int, fields: dict) -> tuple[dict, object]:
    out = {name: [] for name in (*fields, "wall_ms")}
    result = None
    for rep in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        result = call()
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.timing()
        if rep:
            for name, field in fields.items():
                out[name].append(t[field])
            out["wall_ms"].append(wall)
    return {k: spread(v) for k, v in out.items()}, result


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, choices=(150, 5160))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "agreement_timing.jsonl")
    args = ap.parse_args()

    import round_robin_engine_stub as stub
    from farkle_ii_amd import structure_agreement as sa
    from farkle_ii_amd.backend import Engine

    reference = json.loads(GOLDEN.read_text())["meta"] if GOLDEN.exists() else {}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    x, y = ranks(POPULATION)
    with Engine(0) as eng:
        device = eng.device_info()["arch"]
        for n in (150, 5160):
            if args.only not in (None, n):
                continue
            win, ts = x[:n].copy(), y[:n].copy()
            win[3] = ts[7] = 0
            eng.rr_counts_reset()
            eng.rr_counts_add(stub.random_valid_table(n, 5), states(n), GAMES, 2 * GAMES)
            inference, inferred = timed(lambda: eng.rr_inference(want_strategies=False, **PARAMS), eng, args.reps, {"device_ms": "play_ms"})
            fields = {"device_ms": "play_ms", "pair_pass_ms": "perm_ms"}
            counted, bare = timed(lambda: eng.rr_agreement(win, ts, want_codes=False, **PARAMS), eng, args.reps, fields)
            coded, full = timed(lambda: eng.rr_agreement(win, ts, **PARAMS), eng, args.reps, fields)
            eng.rr_counts_reset()
            if not (np.array_equal(bare["class_counts"], inferred["class_counts"]) and np.array_equal(bare["counts"], full["counts"])
                    and np.array_equal(sa.pair_counts(full["codes"], np.zeros(len(full["codes"]), np.uint8))[5:7], full["counts"][5:7])):
                raise SystemExit(f"n = {n}: the timed calls disagree")
            line = {"what": f"rr_agreement_{n}", "strategies": n, "pairs": n * (n - 1) // 2, "reps": args.reps, "rr_inference": inference,
                    "rr_agreement_counts_only": counted, "rr_agreement_with_codes": coded,
                    "counts": {name: int(v) for name, v in zip(sa.COUNT_NAMES, full["counts"])}, "device": device, "commit": args.commit}
            if n == 150 and reference:
                line["reference_pair_agreement_seconds_for_context"] = reference.get("reference_pair_agreement_seconds_family_150")
            print(json.dumps(line), flush=True)
            with args.out.open("a") as fh:
                fh.write(json.dumps(line) + "\n")
        concordance, counts = timed(lambda: eng.rank_concordance(x, y), eng, args.reps, {"device_ms": "play_ms"})
        line = {"what": f"rank_concordance_{POPULATION}", "items": POPULATION, "pairs": POPULATION * (POPULATION - 1) // 2, "reps": args.reps,
                "rank_concordance": concordance, "counts": {name: int(v) for name, v in zip(sa.CONCORDANCE_NAMES, counts)},
                "kendall": sa.kendall_from_counts(counts, POPULATION), "equals_host_statement": bool(np.array_equal(counts, sa.concordance_counts(x, y))),
                "device": device, "commit": args.commit}
        print(json.dumps(line), flush=True)
        with args.out.open("a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
