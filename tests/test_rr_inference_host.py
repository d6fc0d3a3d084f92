"""The statistics of the round-robin inference on the CPU: ``ri_score_test``, ``ri_stat_at`` and ``ri_interval`` of
csrc/fk_rr_inference.h (plain ``__host__ __device__`` C++, built into tests/native/rr_inference_host_check.hip without a GPU and
without the oracle) against the literal restatement of the reference's h2h_inference.py :68-277 in tests/rr_inference_literal.py."""
from __future__ import annotations

import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy.stats import norm

import rr_inference_literal as lit

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "rr_inference_host_check.hip"
ALPHAS = (0.02, 0.02 / 11_175, 0.02 / 13_310_220)  # ordinary; Bonferroni over the production family and over the full grid
# The statistic at a difference: the header cubes and squares by multiplication where the reference raises to a power (one rounding
# apart in q and in p^3), and that relative 2^-52 reaches the constrained rate through acos, whose error near a cosine of +-1 is the
# SQUARE ROOT of its argument's (d acos x = dx / sqrt(1 - x^2)): sqrt(4 x 2^-52) = 3e-8 in the angle, a third of it times 2 p <= 2
# in the rate, and the rate enters the statistic through sqrt(variance).  1e-7 relative (absolute under 1) bounds that; it is the
# reference's own conditioning, not a property of the header, and the interval bounds below are held to their own, much tighter bound.
STAT_RTOL = 1e-7


def cases() -> list[tuple[int, int, int, int]]:
    out = []
    for n in (1, 2, 3, 7):
        out += [(c1, n, c2, n) for c1 in range(n + 1) for c2 in range(n + 1)]
    rng = np.random.default_rng(20260)
    for n in (37, 200, 2191):
        out += [(int(a), n, int(b), n) for a, b in rng.integers(0, n + 1, size=(60, 2))]
    for n in (1, 2, 3, 7, 37, 200, 2191):
        out += [(0, n, 0, n), (n, n, n, n), (0, n, n, n), (n, n, 0, n), (n // 2, n, n // 2, n), ((n + 1) // 2, n, (n + 1) // 2, n)]
    out += [(int(a), 37, int(b), 74) for a, b in zip(rng.integers(0, 38, size=20), rng.integers(0, 75, size=20))]
    out += [(0, 37, 0, 74), (37, 37, 74, 74), (0, 37, 74, 74), (37, 37, 0, 74), (18, 37, 36, 74), (20, 74, 10, 37)]
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("rr_inference") / "rr_inference_host_check"
    # host side only (the checker launches no kernel), as tests/test_round_robin_host.py builds its checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True,
                   capture_output=True, text=True)
    return exe


@pytest.mark.parametrize("alpha", ALPHAS)
def test_header_statistics_against_the_literal_restatement(checker, alpha):
    crit = float(norm.isf(alpha / 2.0))
    todo = cases()
    text = "".join(f"{c1} {n1} {c2} {n2} {crit.hex()}\n" for c1, n1, c2, n2 in todo)
    out = subprocess.run([str(checker)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(todo)
    worst_bound = worst_stat = 0.0
    for case, line in zip(todo, out):
        got = [float.fromhex(v) for v in line.split()]
        assert len(got) == 12
        difference, null_proportion, z, _ = lit.score_test(*case)
        # bit-equal: z, difference, null_proportion
        assert (got[0].hex(), got[1].hex(), got[2].hex()) == (z.hex(), difference.hex(), null_proportion.hex()), case
        for d, g in zip(lit.DIFFERENCES, got[3:8]):
            want = lit.stat_at(*case, d)
            if math.isinf(want) or math.isinf(g):
                assert g == want, (case, d)
            else:
                err = abs(g - want) / max(1.0, abs(want))
                worst_stat = max(worst_stat, err)
                assert err <= STAT_RTOL, (case, d, g, want)
        c1, n1, c2, n2 = case
        want_bounds = (*lit.interval(c1, n1, c2, n2, alpha), *lit.interval(c2, n2, c1, n1, alpha))
        for g, want in zip(got[8:], want_bounds):
            worst_bound = max(worst_bound, abs(g - want))
            assert abs(g - want) <= lit.BOUND_TOL, (case, alpha, got[8:], want_bounds)
        assert got[8] <= difference <= got[9] and got[10] <= -difference <= got[11], case  # the estimate lies inside
        if difference != 0.0:  # the swap rule of :245-253: one side is computed, the other is its mirror image
            assert (got[10], got[11]) == (-got[9], -got[8]), case
    print(f"alpha {alpha:g}: largest bound distance {worst_bound:.3g}, largest statistic distance {worst_stat:.3g} over {len(todo)} cases")
