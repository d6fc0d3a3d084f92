"""CPU check of the roll step's back end: `fk_device.h` is __host__ __device__, so the form the game kernels run
(`roll_back_end50`: counters from the discard byte's ready-made bits, the decision as lane-mask algebra, the bank from the
decision's own entry term, highest_turn as a packed maximum) is compared on the host with its readable statement
(`roll_back_end50_decoded`), each followed by the two-seat table advance, over 923 multisets x dice rolled x the 144 valid
flag sets x thresholds x turn scores x game states; every discard-table byte's new bits are checked against its d5 / d1
fields.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_roll_back_end_matches_decoded_form_on_host(tmp_path):
    exe = tmp_path / "roll_back_end_host_check"
    src = ROOT / "tests" / "native" / "roll_back_end_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread", "-o", str(exe), str(src)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "multisets 923" in out.stdout and "bad_regs 0 bad_over 0 bad_table 0 bad_derived 0 bad_bits 0" in out.stdout
