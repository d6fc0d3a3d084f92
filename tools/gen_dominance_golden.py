#!/usr/bin/env python3
"""Record tests/golden/dominance_vectors.json: the reference's own dominance digest on the cases of tests/dominance_cases.py.

Build container only (it imports the upstream reference through oracle/ref_import.py).  For every case the reference's
``_edge_frames``, ``_graph_structure``, ``_descriptive_scores``, ``_front_frame``, ``_cycle_frame`` and the summary of
``build_dominance_outputs`` run on an inference frame laid out from the case's arrays; the four results are stored as data — a frame
of at most ``FULL_ROWS_LIMIT`` rows value by value with floats as the hex of their bits, a larger one as columns, dtypes, row count
and the SHA-256 of the same serialisation (tests/dominance_cases.py: ``frame_golden``).  The inputs are not stored: the cases are
seeded and a digest of each case's arrays pins them.

    python tools/gen_dominance_golden.py            # rewrite the file
    python tools/gen_dominance_golden.py --check    # compare with the file, exit 1 on a difference
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "oracle")]
GOLDEN = ROOT / "tests" / "golden" / "dominance_vectors.json"
FAMILY_HASH = "dominance-test-family"


def inference_frame(c: dict):
    """The columns ``_read_inference`` requires, from a case."""
    import pandas as pd

    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd.rr_inference import DECISION_CLASSES

    _, i, j = rr.pair_ids(c["n"])
    ids, st, cls = c["ids"], c["strategies"], c["cls"]
    completion = st[:, 8] / st[:, 7]
    data = {"family_hash": FAMILY_HASH, "pair_id": np.arange(len(cls), dtype=np.int64), "strategy_a": ids[i], "strategy_b": ids[j], "d_ab": c["d_ab"],
            "balanced_a_win_rate_alias": c["rate"], "simultaneous_d_low": c["low"], "simultaneous_d_high": c["high"], "holm_reject": cls < 4,
            "practical_delta": c["delta"], "decision_class": np.asarray(DECISION_CLASSES, dtype=object)[cls], "pair_claim_eligible": cls != 6}
    for side, rows in (("a", i), ("b", j)):
        data[f"strategy_{side}_completion_rate"] = completion[rows]
        data[f"strategy_{side}_operationally_viable"] = st[rows, 10] != 0
        data[f"strategy_{side}_inferentially_viable"] = st[rows, 11] != 0
    return pd.DataFrame(data)


def reference_digest(c: dict) -> dict:
    """The reference's four results for one case (the statements of ``build_dominance_outputs`` between reading and writing)."""
    from farkle.analysis import dominance as ref

    inference = inference_frame(c)
    nodes = set(inference["strategy_a"].astype(str)) | set(inference["strategy_b"].astype(str))
    scores_in = {str(k): float(v) for k, v in c["scores"].items()}
    edges, practical_edges, statistical_edges = ref._edge_frames(inference)
    practical = ref._graph_structure(nodes, practical_edges, "practical")
    statistical = ref._graph_structure(nodes, statistical_edges, "statistical")
    scores = ref._descriptive_scores(inference, nodes, practical_edges, statistical_edges, scores_in)
    fronts = ref._front_frame(scores, practical, statistical)
    cycles = ref._cycle_frame(practical, statistical, edges, practical_edges, statistical_edges)
    winners = sorted(s for s in nodes if bool(scores.loc[scores["strategy"].eq(s), "candidate_claim_eligible"].iloc[0])
                     and sum(w == s for w, _ in practical_edges) == len(nodes) - 1)
    decision_counts = inference["decision_class"].astype(str).value_counts().to_dict()
    summary = {
        "family_hash": FAMILY_HASH, "finalist_count": len(nodes), "unordered_pair_count": len(inference),
        "decision_counts": {str(k): int(v) for k, v in decision_counts.items()},
        "practical_edge_count": len(practical_edges), "statistical_edge_count": len(statistical_edges),
        "practical_cycle_group_count": len(practical.cycles), "statistical_cycle_group_count": len(statistical.cycles),
        "practical_front_count": max(practical.fronts.values()), "statistical_front_count": max(statistical.fronts.values()),
        "unique_best": winners[0] if winners else None, "unique_best_claim_permitted": bool(winners),
        "unique_best_rule": "direct_practical_dominance_over_every_other_finalist",
        "operationally_nonviable_candidates": sorted(scores.loc[~scores["operationally_viable"].astype(bool), "strategy"].astype(str)),
        "inferentially_nonviable_candidates": sorted(scores.loc[~scores["inferentially_viable"].astype(bool), "strategy"].astype(str)),
        "display_order_is_inferential": False,
    }
    return {"edges": edges, "fronts": fronts, "cycles": cycles, "summary": summary}


def input_digest(c: dict) -> str:
    h = hashlib.sha256()
    for name in ("ids", "cls", "low", "high", "rate", "d_ab", "strategies"):
        h.update(np.ascontiguousarray(c[name]).tobytes())
    h.update(json.dumps(sorted(c["scores"].items())).encode())
    return h.hexdigest()


def record() -> dict:
    import ref_import

    import dominance_cases as cases

    ref_import.import_reference()
    sys.setrecursionlimit(5000)  # (the reference's component search recurses once per node of a chain)
    out = {}
    for name, c in cases.all_cases().items():
        started = time.perf_counter()
        got = reference_digest(c)
        out[name] = {"inputs_sha256": input_digest(c), "summary": got["summary"],
                     **{key: cases.frame_golden(got[key]) for key in ("edges", "fronts", "cycles")}}
        print(f"{name}: n = {c['n']}, reference {time.perf_counter() - started:.2f} s", file=sys.stderr)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    text = json.dumps(record(), indent=1, sort_keys=True) + "\n"
    if args.check:
        same = GOLDEN.exists() and GOLDEN.read_text() == text
        print("golden file reproduced" if same else "golden file differs", file=sys.stderr)
        return 0 if same else 1
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    GOLDEN.write_text(text)
    print(f"wrote {GOLDEN} ({len(text)} bytes)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
