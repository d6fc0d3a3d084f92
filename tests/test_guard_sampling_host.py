"""CPU check of the sampled guard bands of the two-seat lean game-kernel instances (csrc/fk_device.h, round 12): these instances test the
three u16 counter bands every ``RG_SAMPLE_TRIPS`` trips of a wave and where a game ends, where every other instance tests them in every
roll.  tests/native/guard_sampling_host_check.hip drives the pure pieces on the host: the per-roll half and the sampled half together say
what ``roll_guards50`` says; over a window of ``RG_SAMPLE_TRIPS`` rolls of worst-case growth from every start around a band and around
65 535 - 6 K no field wraps, and whatever went beyond a band inside the window is flagged at its end; the game-end test flags a state iff
a field of either record, the loser's included, or ``highest_turn`` is beyond its band.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_sampled_guard_bands_on_host(tmp_path):
    exe = tmp_path / "guard_sampling_host_check"
    src = ROOT / "tests" / "native" / "guard_sampling_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for part in ("bad_split 0", "wrapped 0", "grew_more 0", "missed 0", "bound 1", "bad_end 0", "highest_fits 1"):
        assert part in out.stdout, out.stdout
