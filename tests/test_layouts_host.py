"""CPU check of the composite device-buffer layouts: csrc/fk_layouts.h is plain host arithmetic, so tests/native/layouts_host_check.hip
evaluates each struct without a GPU, and every offset must equal the formula the engine used before the structs existed (when the same
offsets were derived again at the ensure, at the kernel arguments and at the copies home).  The formulae below are literal copies of that
code: g_sc .. g_u64 and the spill size, r_gs / r_tot / r_u64, shuffle_at, and par_doubles with the d_observed .. d_expected_across chain.
No GPU, no oracle."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "layouts_host_check.hip"
N_COUNTS = 4  # fkg::N_COUNTS


def game_stats(S, rb, mb, cap):
    g_sc = 0
    g_sr = g_sc + S * N_COUNTS
    g_sru = g_sr + S * rb
    g_ssp = g_sru + S * mb
    g_gc = g_ssp + S * mb
    g_gr = g_gc + N_COUNTS
    g_gru = g_gr + rb
    g_cnt = g_gru + mb
    g_u64 = g_cnt + 1
    return [g_sc, g_sr, g_sru, g_ssp, g_gc, g_gr, g_gru, g_cnt, g_u64, g_u64 * 8, g_u64 * 8 + max(cap, 1) * 12]


def rare(S, sb):
    r_gs = S * sb
    r_tot = r_gs + sb
    r_u64 = r_tot + 1
    return [0, r_gs, r_tot, r_u64]


def fingerprints(game_seed_bytes, shuffle_seed_bytes):
    shuffle_at = (game_seed_bytes + 255) & ~255
    return [0, shuffle_at, shuffle_at + shuffle_seed_bytes]


def root_params(n_k, S, joint):
    by_k = n_k * S
    par_doubles = n_k + (2 * by_k + 2 * S if joint else 0)
    d_weights = 0
    d_observed = d_weights + n_k
    d_expected = d_observed + by_k
    d_observed_across = d_expected + by_k
    d_expected_across = d_observed_across + S
    return [d_weights, d_observed, d_expected, d_observed_across, d_expected_across, par_doubles]


CASES = (
    [("game_stats", a, game_stats(*a)) for a in [(1, 1, 1, 0), (2, 3, 5, 1), (2, 3, 5, 7), (5160, 201, 400, 0), (5160, 201, 400, 100000)]]
    + [("rare", a, rare(*a)) for a in [(1, 1), (5160, 1), (1, 257), (5160, 257)]]
    + [("fingerprints", a, fingerprints(*a)) for a in [(0, 12), (1, 12), (65, 12), (256, 4), (65, 0)]]
    + [("root_params", (n_k, S, int(joint)), root_params(n_k, S, joint)) for n_k in (1, 3) for S in (1, 7) for joint in (False, True)]
)


@pytest.mark.skipif(not (shutil.which(HIPCC) or Path(HIPCC).exists()), reason="hipcc not available")
def test_every_layout_equals_the_formulae_it_replaced(tmp_path):
    exe = tmp_path / "layouts_host_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True,
                   capture_output=True, text=True)
    text = "".join(f"{kind} {' '.join(str(v) for v in args)}\n" for kind, args, _ in CASES)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    wrong = [f"{kind}{args}: {line} != {want}" for (kind, args, want), line in zip(CASES, lines) if [int(v) for v in line.split()] != want]
    assert not wrong, "\n".join(wrong)
    # a layout's parts do not overlap and fill it: the offsets rise and the last part ends at the total
    for kind, args, want in CASES:
        if kind == "game_stats":
            assert want[:9] == sorted(want[:9]) and want[8] == want[7] + 1
