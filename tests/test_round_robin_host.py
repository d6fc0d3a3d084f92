"""The pair numbering of the round robin on the CPU: ``rr_unrank`` of csrc/fk_round_robin.h (plain ``__host__ __device__`` C++, built
into tests/native/round_robin_host_check.hip without a GPU and without the oracle) and ``round_robin.unrank`` (NumPy), both against
the enumeration of ``itertools.combinations(range(n), 2)`` — the order in which the reference's ``_schedule_frame`` numbers pairs."""
from __future__ import annotations

import os
import shutil
import subprocess
from itertools import combinations
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "round_robin_host_check.hip"
SMALL = (2, 3, 4, 5, 64, 65, 1000)         # every pair, by enumeration
LARGE = (5160, 65_536, 1_048_576)          # the first and last pair of every row


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_rr_unrank_against_enumeration(tmp_path):
    exe = tmp_path / "round_robin_host_check"
    # host side only (the checker launches no kernel), as tests/launch_plan_cases.py builds the planner's checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True,
                   capture_output=True, text=True)
    text = "".join(f"{n} 0\n" for n in SMALL) + "".join(f"{n} 1\n" for n in LARGE)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line]
    want = [(n, n * (n - 1) // 2, 0) for n in SMALL] + [(n, 2 * (n - 1), 0) for n in LARGE]
    assert got == want


@pytest.mark.parametrize("n", SMALL)
def test_python_unrank_against_itertools(n):
    from farkle_ii_amd import round_robin as rr

    want = np.array(list(combinations(range(n), 2)), dtype=np.int64)
    assert rr.pair_count(n) == len(want)
    pid, i, j = rr.pair_ids(n)
    assert np.array_equal(pid, np.arange(len(want))) and np.array_equal(i, want[:, 0]) and np.array_equal(j, want[:, 1])
    gi, gj = rr.unrank(n, len(want) - 1)  # a scalar
    assert (int(gi), int(gj)) == (n - 2, n - 1)


@pytest.mark.parametrize("n", LARGE)
def test_python_unrank_row_ends_of_large_tables(n):
    from farkle_ii_amd import round_robin as rr

    rows = np.arange(n - 1, dtype=np.int64)
    first = rows * (2 * n - rows - 1) // 2
    last = first + (n - rows - 2)
    for pid, want_j in ((first, rows + 1), (last, np.full(n - 1, n - 1))):
        i, j = rr.unrank(n, pid)
        assert np.array_equal(i, rows) and np.array_equal(j, want_j)


def test_python_unrank_refuses_what_is_not_a_pair():
    from farkle_ii_amd import round_robin as rr

    with pytest.raises(ValueError, match="at least two strategies"):
        rr.unrank(1, 0)
    with pytest.raises(ValueError, match=r"pair ids must be in \[0, 10\)"):
        rr.unrank(5, 10)
    with pytest.raises(ValueError, match="pair ids"):
        rr.unrank(5, -1)
