"""The register budget of the two-seat game-kernel instances, read from the built library's code object (no GPU): the 768-thread blocks
seat six waves per SIMD only while an instance allocates at most 80 VGPRs, and with `amdgpu_waves_per_eu(6)` the compiler meets that
limit by spilling to scratch, silently.  The flat hand-over (round 10) took the tournament instance from 71 to 79 VGPRs: the next
register it needs must show up here, not as scratch traffic in the roll loop."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

LLVM = Path("/opt/rocm/llvm/bin")
TOOLS = [LLVM / "llvm-objcopy", LLVM / "clang-offload-bundler", LLVM / "llvm-readelf"]


@pytest.mark.skipif(not all(t.exists() or shutil.which(t.name) for t in TOOLS), reason="LLVM binary tools not available")
def test_two_seat_instances_fit_six_waves_without_scratch(tmp_path):
    from farkle_ii_amd import backend

    lib = backend.build_library()
    fatbin, code = tmp_path / "fatbin", tmp_path / "gfx950.co"
    subprocess.run([str(TOOLS[0]), f"--dump-section=.hip_fatbin={fatbin}", str(lib), str(tmp_path / "copy.so")], check=True, capture_output=True)
    subprocess.run([str(TOOLS[1]), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fatbin}",
                    f"--output={code}"], check=True, capture_output=True)
    notes = subprocess.run([str(TOOLS[2]), "--notes", str(code)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for entry in notes.split("  - .agpr_count:")[1:]:  # one metadata entry per kernel
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        if not re.search(r"fk_play_kernelILi768ELb1ELi6ELj\d+ELb0ELb[01]ELi2EEE", name):
            continue
        seen += 1
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        assert scratch == 0 and vgprs <= 80, (name, vgprs, scratch)
    assert seen == 6  # three flag forms x (tournament / game-list instance, H2H block instance)
