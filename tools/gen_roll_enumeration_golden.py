"""TEST INFRASTRUCTURE ONLY — write tests/golden/roll_enumeration.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

``enumerate_ordered_roll_outcomes()`` of the reference (src/farkle/analysis/roll_enumeration.py:56-110): the exact distribution of
(max_immediate_score, scoring_dice) over the 6^d ordered outcomes of d = 1 .. 6 dice and its per-dice-count summary.  Both frames are
stored as data: column names in order, pandas dtypes, rows; floats as ``float.hex()`` strings so that the comparison is by bit
pattern.

    python tools/gen_roll_enumeration_golden.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
from ref_import import import_reference  # noqa: E402

import_reference()
from farkle.analysis.roll_enumeration import enumerate_ordered_roll_outcomes  # noqa: E402

OUT = HERE.parent / "tests" / "golden" / "roll_enumeration.json"


def frame_as_data(frame) -> dict:
    def cell(v):
        if isinstance(v, float):
            return v.hex()
        return v.item() if hasattr(v, "item") else v

    return {"columns": list(frame.columns), "dtypes": [str(t) for t in frame.dtypes],
            "rows": [[cell(v) for v in row] for row in frame.itertuples(index=False, name=None)]}


def main() -> None:
    distribution, summary = enumerate_ordered_roll_outcomes()
    per_dice = distribution.groupby("dice_count").size().tolist()
    assert len(distribution) == 127 and per_dice == [3, 6, 12, 22, 35, 49], per_dice
    assert int(distribution["max_immediate_score"].max()) == 3000
    assert summary["farkle_count"].tolist() == [4, 16, 60, 204, 600, 1080]
    out = {"floats": "float.hex()", "distribution": frame_as_data(distribution), "summary": frame_as_data(summary)}
    OUT.write_text(json.dumps(out, separators=(",", ":")))
    print(OUT, OUT.stat().st_size, "bytes;", len(distribution), "distribution rows", per_dice)


if __name__ == "__main__":
    main()
