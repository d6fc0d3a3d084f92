"""The inputs of ``test_analysis_scale_gpu.py`` reach the regimes they are there for — shown on the reference result alone (the
oracle-backed stubs), without a GPU: every rare-event case has events beyond the game id at which its code path starts, fewer
events than games (or exactly the completed games in the dense case) and no spill; the 5 160-strategy pair case has more than
65 536 pairs, the 300-strategy one pairs of two and more games with both unpaired columns in use."""
from __future__ import annotations

import pytest

import analysis_scale_cases as asc


@pytest.mark.parametrize("name", list(asc.RARE_CASES))
def test_rare_event_case_reaches_its_regime(name):
    fig = asc.check_rare_preconditions(name)
    print(name, fig)
    c = asc.RARE_CASES[name]
    assert fig["games"] == {"slots_multiwave": 103_200, "two_tiles_mixed": 265_740, "two_tiles_dense": 265_740, "two_tiles_k3": 264_880,
                            "grid_stride": 528_900, "hot_cold_k12": 17_200}[name]
    if c["k"] <= 3:  # (twelve seats: some seat reaches 2 000 points long before round 200)
        assert fig["safety"] > 0  # safety-limit games: never flagged by a margin, counted in the second-score histograms
    if not c["dense"]:
        assert 0 < fig["multi_only"] < fig["events"]  # both kinds of event: multi alone, and a margin threshold
    else:
        assert fig["multi_only"] == 0 and fig["events"] > 65_536  # more than the default event capacity
    if name == "grid_stride":
        assert fig["safety"] > 100_000  # max_rounds = 6: about a fifth of the games end at the limit


def test_the_permutation_image_blocks_are_short_and_the_last_one_ragged():
    """What `slots` of the host code gives at the production table: min(512, 160 KiB / 2 S) = 15 shuffles per block (a chunk's
    blocks count from the chunk's first shuffle), so every one-chunk case spans at least three blocks and ends inside one."""
    S = len(asc.table(asc.GRID, 2))
    slots = min(512, (160 << 10) // (2 * S))
    assert S == 5160 and slots == 15
    spans = [c["n_sh"] for c in asc.RARE_CASES.values()] + [c["end"] - c["begin"] for c in asc.SEAT_CASES.values() if c["S"] == S]
    assert all(n > 2 * slots and n % slots for n in spans)


@pytest.mark.parametrize("name", list(asc.SEAT_CASES))
def test_seat_case_reaches_its_regime(name):
    fig = asc.check_seat_preconditions(name)
    print(name, fig)
    assert fig["games"] == {"pairs_5160": 103_200, "pairs_300": 270_000, "counts_k5": 41_280}[name]
    if name == "pairs_5160":
        assert fig["pairs"] <= fig["games"] and asc.ids(5160)[0] == 5159  # ranks of 13 bits, in the reverse of the table's order
    if name == "pairs_300":
        assert fig["pairs"] <= 300 * 299 // 2 and fig["safety"] > 0
