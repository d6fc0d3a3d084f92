"""CPU check of the two-seat table advance on lane masks: `fk_device.h` is __host__ __device__, so `advance2_flags50` on lane masks (the form the
two-seat lean game kernels run on their carried 64-lane flag masks) is compared on the host with `advance2_table50`, lane by lane, over
every combination of its five boolean inputs, three lane orders, max_rounds 0 / 1 / 2 and rounds below, at and above the limit.  The
program is built twice: plainly, and with the address and undefined-behaviour sanitizers on the host code.  No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = ROOT / "tests" / "native" / "advance2_masks_host_check.hip"


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_advance2_masks_match_table_form_on_host(tmp_path, sanitize):
    exe = tmp_path / "advance2_masks_host_check"
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-g", "-std=c++17", *flags, "-o", str(exe), str(SRC)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases 1152 " in out.stdout and out.stdout.rstrip().endswith("bad 0"), out.stdout
