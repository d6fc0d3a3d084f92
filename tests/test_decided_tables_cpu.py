"""The decided-outcome tables of `decided_table_cases.py` on the CPU oracle alone: each case IS what `test_decided_tables_gpu.py`
takes it for — batches without a completed game, one strategy that takes every win, mirrored pairs of all three decided kinds,
strategies whose ratio sums stay +0.0, all wins on a slice edge of the tally reduce — so that the GPU tests cannot pass by having
lost their subject.  Every figure a condition reads is printed before it is asserted (``pytest -s``).

One condition is stated narrower than it was first asked for.  "``game_second`` of half64 at two seats has all its mass in bin 0"
cannot hold under any target, round limit or seed: half of that table banks, two bankers meet in a quarter of the games (755 of
3 072 here) and the loser of such a game keeps its points (518 of the 755 lose with 50 points or more).  What does hold, and is
asserted exactly: a never-banker's score is 0 in every row, so every game that seats one has a second score of 0 — the whole
``strategy_second`` row of each never-banker is its bin 0 — and the mass of ``game_second`` beyond bin 0 is the banker-against-banker
games alone; the histogram that IS all bin 0 is none64's (two and four seats) and one64's."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import decided_table_cases as dc  # noqa: E402
from rare_events_engine_stub import Engine as RareStub  # noqa: E402
from seat_analysis_engine_stub import Engine as SeatStub  # noqa: E402

from farkle_ii_amd import game_stats as gs  # noqa: E402


def test_the_builder_leaves_bankers_that_bank_and_the_rest_never_banking():
    for name in dc.TABLES:
        t, base = dc.table(name), dc.base_table(64 if name.endswith("64") else 12)
        never = dc.never_banks(t)
        assert 0 < never.sum() <= len(t) and np.array_equal(t["strategy_id"], base["strategy_id"])
        changed = [n for n in t.dtype.names if not np.array_equal(t[n][~never], base[n][~never])]
        assert changed in ([], ["require_both"]), (name, changed)  # a banker is the grid's row, or that row made to bank
    ids = dc.half12_ids()
    assert sorted(np.argsort(ids)[0::2].tolist()) == dc.half12_bankers() and len(dc.half12_bankers()) == 6
    assert len(set(ids.tolist())) == 12 and not np.array_equal(np.argsort(ids), np.arange(12))
    assert not dc.never_banks(dc.edge_table(0))[0] and dc.never_banks(dc.edge_table(0)).sum() == dc.EDGE_S - 1


@pytest.mark.parametrize("k", dc.SEATS["none64"])
def test_none64_every_game_hits_the_limit(k):
    r = dc.run(RareStub(), "tournament_rare_events", dc.table("none64"), k, **dc.TALLY_BATCHED, rare_target_score=dc.RARE_TARGET)
    tally = r["tally"]
    print("none64 k", k, "wins", tally[..., dc.WINS].sum(), "completed", tally[..., dc.COMPLETED].sum(), "safety per batch",
          tally[:, 0, dc.SAFETY])
    assert tally.shape[0] == 3 and not tally[..., dc.WINS].any() and not tally[..., dc.COMPLETED].any()
    assert np.array_equal(tally[..., dc.SAFETY], np.repeat([[16], [16], [8]], 64, axis=1))
    second = r["rare_events"]["game_second"]
    assert second[0] == 40 * (64 // k) and second.sum() == second[0]  # every second-highest score is 0


def test_one64_a_single_strategy_takes_every_win():
    r = dc.run(SeatStub(), "tournament_lags", dc.table("one64"), 2, 0, dc.LAG_SHUFFLES, dc.LAGS)
    tally, sums = r["tally"][0], r["lag_sums"]
    others = np.delete(np.arange(64), 17)
    print("one64 wins of 17:", tally[17, dc.WINS], "of", tally[17, dc.GAMES], "completed", tally[17, dc.COMPLETED],
          "| (pairs, wx, wy, wxy) per lag:", sums[17][:, [dc.LAG_PAIRS, dc.LAG_WX, dc.LAG_WY, dc.LAG_WXY]].tolist())
    assert tally[17, dc.WINS] > 0 and not tally[others, dc.WINS].any() and (tally[others, dc.GAMES] >= 1).all()
    assert tally[17, dc.WINS] == tally[17, dc.COMPLETED] == tally[:, dc.COMPLETED].sum() // 2  # it wins every game it completes
    assert sums[17, 0, dc.LAG_WXY] > 0                      # lag 1: wins in consecutive shuffles
    assert (sums[17, :2, dc.LAG_WXY] > 0).any()             # lags 1 and 3
    assert not sums[others][:, :, [dc.LAG_WX, dc.LAG_WY, dc.LAG_WXY]].any()
    rare = dc.run(RareStub(), "tournament_rare_events", dc.table("one64"), 2, **dc.HALF64_PAIRS, rare_target_score=dc.RARE_TARGET,
                  thresholds=dc.DENSE_THRESHOLDS)
    completed = int(rare["game_stats"]["game_counts"][gs.COMPLETED])
    print("one64 events", rare["rare_events"]["events"], "completed", completed, "of", 96 * 32, "games")
    assert rare["rare_events"]["events"] == completed and 0 < completed <= 96  # all completed games, a minority: at most one a shuffle
    assert rare["rare_events"]["game_second"][1:].sum() == 0                   # the loser's score is 0 in every game
    # with twenty rounds to play it wins every shuffle: wx = wy = wxy = pairs
    always = dc.run(SeatStub(), "tournament_lags", dc.table("one64"), 2, 0, dc.LAG_SHUFFLES, dc.LAGS, max_rounds=dc.ONE64_ALWAYS_ROUNDS)
    assert always["tally"][0, 17, dc.WINS] == dc.LAG_SHUFFLES
    for col in (dc.LAG_WX, dc.LAG_WY, dc.LAG_WXY):
        assert np.array_equal(always["lag_sums"][17, :, col], [dc.LAG_SHUFFLES - lag for lag in dc.LAGS])


def test_half12_mirrored_pairs_of_every_decided_kind():
    r = dc.run(SeatStub(), "tournament_seat_counts", dc.table("half12"), 2, **dc.HALF12_PAIRS, strategy_ids=dc.half12_ids(), want_mirrored=True)
    kinds = dc.pair_kinds(r["pair_sums"])
    print("half12 pair rows", len(r["pair_sums"]), kinds)
    assert len(r["pair_sums"]) == 66 and all(n >= 1 for n in kinds.values()), kinds
    # 6 x 6 banker / never-banker pairs, the lower ID the banker in some and the never-banker in others; 15 pairs of never-bankers
    assert kinds["all_plus"] + kinds["all_minus"] == 36 and kinds["none_completed"] == 15


@pytest.mark.parametrize("k", dc.SEATS["half64"])
def test_half64_completed_and_limit_games_and_scores_of_zero(k):
    t = dc.table("half64")
    never = np.nonzero(dc.never_banks(t))[0]
    stub = RareStub()
    r = dc.run(stub, "tournament_rare_events", t, k, **dc.HALF64_PAIRS, rare_target_score=dc.RARE_TARGET, thresholds=dc.DENSE_THRESHOLDS,
               want_seat_stats=True)
    counts = r["game_stats"]["game_counts"]
    print("half64 k", k, "games", counts[gs.ATTEMPTED], "completed", counts[gs.COMPLETED], "limit", counts[gs.SAFETY], "events",
          r["rare_events"]["events"], "game_second[0]", r["rare_events"]["game_second"][0])
    assert counts[gs.COMPLETED] >= 1 and counts[gs.SAFETY] >= 1
    # the event list is every completed game (and the limit games in which two seats passed the rare target)
    assert counts[gs.COMPLETED] <= r["rare_events"]["events"] <= counts[gs.COMPLETED] + counts[gs.MULTI_TARGET]
    ratios = r["seat_ratio_sums"][:, never]
    assert ratios.tobytes() == np.zeros_like(ratios).tobytes()  # +0.0, not -0.0
    assert not r["tally"][:, never, dc.WINS].any()
    rows = dc.run(stub, "tournament", t, k, **dc.HALF64_PAIRS, want_rows=True)["rows"]
    assert not rows["seats"]["score"][np.isin(rows["seats"]["strategy"], never)].any()  # a never-banker's score stays 0
    if k == 2:
        # The second-highest score of a two-seat game is the loser's: 0 in every game that seats a never-banker, so the whole
        # histogram row of a never-banker is its bin 0.  (Two bankers leave a loser with points: those games, and no others, are
        # the mass of game_second beyond bin 0.)
        second, per = r["rare_events"]["game_second"], r["rare_events"]["strategy_second"]
        with_never = np.isin(rows["seats"]["strategy"], never).any(axis=1)
        loser = rows["seats"]["score"].min(axis=1)
        print("half64 k 2: games seating a never-banker", int(with_never.sum()), "| games of two bankers", int((~with_never).sum()),
              "of them with a loser below 50 points", int((loser[~with_never] < 50).sum()))
        assert np.array_equal(per[never, 0], np.full(len(never), 96)) and not per[never, 1:].any()
        assert second[0] == with_never.sum() + (loser[~with_never] < 50).sum() and second[0] > second[1:].sum() > 0


@pytest.mark.parametrize("winner", dc.EDGE_WINNERS)
def test_edge1794_all_wins_on_one_slice_edge(winner):
    tally = dc.run(SeatStub(), "tournament", dc.edge_table(winner), 2, **dc.EDGE_RANGE)["tally"]
    others = np.delete(np.arange(dc.EDGE_S), winner)
    print("edge1794 winner", winner, "wins per batch", tally[:, winner, dc.WINS].tolist(), "completed", tally[:, winner, dc.COMPLETED].tolist())
    assert tally.shape[0] == 3 and 5 * (dc.EDGE_S // 2) >= 4096  # batches of the reduce kernel
    assert (tally[:, winner, dc.WINS] > 0).sum() >= 2 and not tally[:, others, dc.WINS].any()
    assert (tally[:, others, dc.SAFETY].sum(axis=0) > 0).all()
