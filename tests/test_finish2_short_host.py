"""CPU check of the two-seat game end in its round-11 form: `finish2_50` is now `finish2_second` (who won, from the two score words) and
`finish2_50_winner` (the metrics, from the winner's record alone), and the tally's sums of squares come from `finish2_square` (a 32-bit
product for the metrics bounded by 65 535).  `tests/native/finish2_short_host_check.hip` compares them on the host with
`finish2_50_decoded` and with the 64-bit product, over every combination of the field extremes, both winners, ties, `final_round` 0 / 1,
and states the two bounds as static assertions.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_short_finish_against_its_decoded_form_on_host(tmp_path):
    exe = tmp_path / "finish2_short_host_check"
    src = ROOT / "tests" / "native" / "finish2_short_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("bad 0", "bad_tie 0", "bad_metric 0", "bad_square 0"):
        assert word in out.stdout, out.stdout
