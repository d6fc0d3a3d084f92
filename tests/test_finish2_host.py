"""CPU check of the two-seat game end: `fk_device.h` is __host__ __device__, so `finish2_50` — the pure function the two-seat lean
game kernels end a game with (completed, winner seat, winner's strategy index, the ten metric values) — is compared on the host with
its readable statement (`finish2_50_decoded`): equal scores (seat 0 wins the tie), every metric at 0 and at its guard-band and field
maximum for winner and loser, a final round against the round limit, and `max_rounds` 0.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_finish2_against_its_decoded_form_on_host(tmp_path):
    exe = tmp_path / "finish2_host_check"
    src = ROOT / "tests" / "native" / "finish2_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad 0" in out.stdout and "bad_tie 0" in out.stdout and "bad_metric 0" in out.stdout
