"""CPU check of the roll step's guards and of the discard table's wide entries: `fk_device.h` is __host__ __device__, so the guard
predicate the game kernels run (`roll_guards50`: the roll limit of a turn and the guard bands of the 16-bit counter fields, as compares
on the packed words) is compared on the host with its readable statement (`roll_guards50_decoded`) over every combination of the
guarded values within two of their limits; every wide discard entry (`discard_lut_entry32`) is checked against the byte entry it
restates, and the back end's wide front end (`roll_back_end50w`) against the byte one.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_roll_guards_and_wide_discard_entries_on_host(tmp_path):
    exe = tmp_path / "roll_guards_host_check"
    src = ROOT / "tests" / "native" / "roll_guards_host_check.hip"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad_guard 0" in out.stdout and "bad_wide 0" in out.stdout and "bad_back 0" in out.stdout
