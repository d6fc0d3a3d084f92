#!/usr/bin/env python3
"""Record tests/golden/agreement_vectors.json: the reference's own method agreement on the cases of tests/agreement_cases.py.

Build container only (it imports the upstream reference through oracle/ref_import.py).  For every case the reference's
``_pair_agreement`` and ``_summary`` run on the case's membership frame, an inference frame laid out from its classes and a root
agreement table with its counts; the results are stored as data — the summary as it is, the pair frame of at most
``FULL_ROWS_LIMIT`` rows value by value, a larger one as columns, dtypes, row count and the SHA-256 of the same serialisation
(tests/agreement_cases.py: ``frame_golden``).  The inputs are not stored: the cases are seeded and a digest of each case's arrays pins
them.  ``meta`` holds the seconds the reference's ``_pair_agreement`` took on ``family_150``; ``--check`` does not compare it.

    python tools/gen_agreement_golden.py            # rewrite the file
    python tools/gen_agreement_golden.py --check    # compare with the file, exit 1 on a difference
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
GOLDEN = ROOT / "tests" / "golden" / "agreement_vectors.json"


def input_digest(c: dict) -> str:
    import agreement_cases as cases

    h = hashlib.sha256()
    for a in (c["ids"], c["cls"], c["root_summary"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(json.dumps(cases.frame_records(c["membership"])["rows"], separators=(",", ":")).encode("utf-8"))
    return h.hexdigest()


def record() -> dict:
    import ref_import

    import agreement_cases as cases

    ref_import.import_reference()
    from farkle.analysis import structure_agreement as ref

    out, meta = {}, {}
    for name, c in cases.all_cases().items():
        started = time.perf_counter()
        pairs = ref._pair_agreement(c["membership"], cases.inference_frame(c))
        seconds = time.perf_counter() - started
        summary = ref._summary(c["membership"], pairs, cases.root_agreement_frame(c), execution_scope=c["execution_scope"])
        out[name] = {"inputs_sha256": input_digest(c), "summary": summary, "pairs": cases.frame_golden(pairs)}
        if name == "family_150":
            meta["reference_pair_agreement_seconds_family_150"] = round(seconds, 3)
        print(f"{name}: n = {c['n']}, population {len(c['membership'])}, reference _pair_agreement {seconds:.2f} s", file=sys.stderr)
    return {"meta": meta, "cases": out}


def dumps(golden: dict) -> str:
    """Indented JSON with every frame row on one line."""
    rows: list[str] = []

    def fold(node):
        if isinstance(node, dict):
            return {k: ([fold_row(r) for r in v] if k == "rows" else fold(v)) for k, v in node.items()}
        return node

    def fold_row(row) -> str:
        rows.append(json.dumps(row, separators=(",", ":")))
        return f"@@ROW{len(rows) - 1}@@"

    text = json.dumps(fold(golden), indent=1, sort_keys=True)
    for k, row in enumerate(rows):
        text = text.replace(f'"@@ROW{k}@@"', row, 1)
    return text + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    golden = record()
    if args.check:
        same = GOLDEN.exists() and json.loads(GOLDEN.read_text())["cases"] == json.loads(dumps(golden))["cases"]
        print("golden file reproduced" if same else "golden file differs", file=sys.stderr)
        return 0 if same else 1
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    text = dumps(golden)
    GOLDEN.write_text(text)
    print(f"wrote {GOLDEN} ({len(text)} bytes)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
