"""CPU check of the exact ordered-roll law: `fk_device.h` is __host__ __device__, so `score_counts` — the scorer the roll census takes a
roll's raw cell from — runs on the host over all 6^d ordered outcomes of d = 1 .. 6 dice, and its cells are compared with the 127 rows
of the reference's enumeration (tests/golden/roll_enumeration.json, tools/gen_roll_enumeration_golden.py).  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import golden_util as gu
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_score_counts_over_all_ordered_outcomes_equals_the_reference_enumeration(tmp_path):
    exe = tmp_path / "roll_enumeration_host_check"
    src = ROOT / "tests" / "native" / "roll_enumeration_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    cells = [tuple(int(v) for v in line[1:]) for line in lines if line[0] == "cell"]
    golden = gu.load("roll_enumeration.json")
    dist, summ = golden["distribution"], golden["summary"]
    col = {name: i for i, name in enumerate(dist["columns"])}
    want = [(r[col["dice_count"]], r[col["max_immediate_score"]], r[col["scoring_dice"]], r[col["ordered_outcome_count"]]) for r in dist["rows"]]
    assert len(want) == 127 and cells == want  # the same cells, in the same order
    scol = {name: i for i, name in enumerate(summ["columns"])}
    totals = [tuple(int(v) for v in line[1:]) for line in lines if line[0] == "total"]
    assert totals == [(r[scol["dice_count"]], r[scol["ordered_outcomes"]], r[scol["farkle_count"]]) for r in summ["rows"]]
    assert [t[2] for t in totals] == [4, 16, 60, 204, 600, 1080]
    assert [line[2] for line in lines if line[0] == "bad"] == ["0"] * 6
