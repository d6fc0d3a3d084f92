"""The roll census without a GPU: the exact ordered-roll enumeration against the reference's (tests/golden/roll_enumeration.json),
``RollCensus.from_events`` against a direct count over the events of tests/trace_oracle.py, the census invariants, and the frames of
``roll_fit`` / ``strategy_turn_table`` on a hand-made census."""
from __future__ import annotations

import math

import census_cases
import golden_util as gu
import numpy as np
import pyoracle as po
import pytest
import trace_oracle

from farkle_ii_amd import roll_census as rc
from farkle_ii_amd import trace

GOLDEN = gu.load("roll_enumeration.json")


def frame_as_data(frame) -> dict:
    """A frame the way tools/gen_roll_enumeration_golden.py stores one: floats as float.hex() (compared by bit pattern)."""
    def cell(v):
        if isinstance(v, float):
            return v.hex()
        return v.item() if hasattr(v, "item") else v

    return {"columns": list(frame.columns), "dtypes": [str(t) for t in frame.dtypes],
            "rows": [[cell(v) for v in row] for row in frame.itertuples(index=False, name=None)]}


def test_enumeration_equals_the_reference_frames_bit_for_bit():
    distribution, summary = rc.enumerate_ordered_roll_outcomes()
    for name, frame in (("distribution", distribution), ("summary", summary)):
        got, want = frame_as_data(frame), GOLDEN[name]
        assert got["columns"] == want["columns"], name
        assert got["dtypes"] == want["dtypes"], name
        assert len(got["rows"]) == len(want["rows"])
        for i, (a, b) in enumerate(zip(got["rows"], want["rows"])):
            assert a == b, (name, i)  # row order, every column, floats by their hex
    assert len(distribution) == 127 and distribution.groupby("dice_count").size().tolist() == [3, 6, 12, 22, 35, 49]
    assert int(distribution["max_immediate_score"].max()) == 3000 and summary["farkle_count"].tolist() == [4, 16, 60, 204, 600, 1080]
    exact = rc.exact_cells()
    assert exact.shape == (6, 61, 7) and exact.sum(axis=(1, 2)).tolist() == [6 ** d for d in range(1, 7)] and int((exact > 0).sum()) == 127


@pytest.fixture(scope="module")
def traced():
    """The small list's parts, traced once by the oracle helper: (table, [(events, begin, rows, seat_strategy, k)])."""
    table, parts = census_cases.small_list()
    out = []
    for coords, ss, k, target, max_rounds in parts:
        rows, begin, events = trace_oracle.pinned(coords, table, ss, k, target, max_rounds)
        out.append((events, begin, rows, np.asarray(ss).reshape(len(coords), k), k))
    return table, out


def direct_count(table, traced_parts, turn_bins):
    """The census counted one event at a time; a roll's raw score and scoring dice from the ORACLE's scorer with a strategy that
    discards nothing."""
    S = len(table)
    plain = np.zeros(1, dtype=po.STRATEGY_DTYPE)  # smart_five = smart_one = 0: default_score returns the raw roll
    cells = np.zeros((6, 61, 7), np.int64)
    dice = np.zeros((S, 6, 3), np.int64)
    turns = np.zeros((S, 3), np.int64)
    hist = np.zeros((S, turn_bins), np.int64)
    for events, begin, rows, ss, k in traced_parts:
        all_faces = trace.faces(events)
        for g in range(len(begin) - 1):
            for i in range(int(begin[g]), int(begin[g + 1])):
                e = events[i]
                s = int(ss[g, int(e["seat"])])
                faces = all_faces[i]
                n = len(faces)
                pts, used, _, d5, d1 = po.default_score(faces, 0, plain)
                assert d5 == 0 and d1 == 0
                cells[n - 1, pts // 50, used] += 1
                dice[s, n - 1, 0] += 1
                dice[s, n - 1, 1] += pts == 0
                dice[s, n - 1, 2] += used == n
                if not int(e["flags"]) & trace.EV_ROLL_AGAIN:
                    turns[s, 0] += 1
                    turns[s, 1] += int(e["points"]) == 0
                    turns[s, 2] += int(e["turn_score"])
                    hist[s, min(int(e["turn_score"]) // 50, turn_bins - 1)] += 1
    return rc.RollCensus(cells, dice, turns, hist)


def test_the_small_list_holds_what_the_census_must_tell_apart(traced):
    """Asserted from the oracle's events before anything is compared: the list exercises the raw / after-discard difference, a six-dice
    all-scoring roll, an auto-hot-dice roll, and a turn in the clamp bin at turn_bins = 8."""
    table, parts = traced
    events = np.concatenate([p[0] for p in parts])
    score50_of, used_of = rc._outcome_cells()
    raw = score50_of[events["dice"].astype(np.int64)].astype(np.int64) * 50
    raw_used = used_of[events["dice"].astype(np.int64)]
    assert ((events["points"] != raw) & (events["discards"] != 0)).any()            # a discard changed the roll's score
    assert not ((events["points"] != raw) & (events["discards"] == 0)).any()
    assert ((trace.n_dice(events) == 6) & (raw_used == 6)).any()                    # six dice, all scoring
    assert trace.auto_hot(events).any()                                             # a roll continued by auto_hot_dice
    last = ~trace.rolls_again(events)
    assert (events["turn_score"][last] // 50 >= 7).any()                            # a turn in the clamp bin at turn_bins = 8
    assert any(len(p[1]) == 2 and p[1][-1] == 0 for p in parts)                     # the max_rounds = 0 game: no event


@pytest.mark.parametrize("turn_bins", [8, 256])
def test_from_events_equals_a_direct_count_and_keeps_the_invariants(traced, turn_bins):
    table, parts = traced
    S = len(table)
    census = rc.RollCensus.zeros(S, turn_bins)
    for events, begin, rows, ss, k in parts:
        census = census.merge(rc.RollCensus.from_events(events, begin, ss, S, turn_bins))
    want = direct_count(table, parts, turn_bins)
    for name in ("roll_cells", "strategy_dice", "strategy_turns", "turn_hist"):
        assert np.array_equal(getattr(census, name), getattr(want, name)), name
    # the invariants
    for n in range(6):
        cells = census.roll_cells[n]
        assert census.strategy_dice[:, n, 0].sum() == cells.sum()
        assert census.strategy_dice[:, n, 1].sum() == cells[0].sum()
        assert census.strategy_dice[:, n, 2].sum() == cells[:, n + 1].sum()
    assert census.outside_support() == 0 and not census.roll_cells[rc.exact_cells() == 0].any()
    assert np.array_equal(census.strategy_dice[:, :, 1].sum(axis=1), census.strategy_turns[:, 1])
    assert np.array_equal(census.turn_hist.sum(axis=1), census.strategy_turns[:, 0])
    if turn_bins == 8:
        assert census.turn_hist[:, 7].sum() > 0
    # per strategy: rolls, farkles and turns are the sums of the oracle rows' counters
    rolls, farkles, n_turns = (np.zeros(S, np.int64) for _ in range(3))
    for events, begin, rows, ss, k in parts:
        seats = rows["seats"]
        np.add.at(rolls, seats["strategy"].reshape(-1), seats["rolls"].reshape(-1).astype(np.int64))
        np.add.at(farkles, seats["strategy"].reshape(-1), seats["farkles"].reshape(-1).astype(np.int64))
        np.add.at(n_turns, seats["strategy"].reshape(-1), seats["n_turns"].reshape(-1).astype(np.int64))
    assert np.array_equal(census.strategy_dice[:, :, 0].sum(axis=1), rolls)
    assert np.array_equal(census.strategy_dice[:, :, 1].sum(axis=1), farkles)
    assert np.array_equal(census.strategy_turns[:, 0], n_turns)


def test_from_events_refuses_what_is_not_a_census():
    table, parts = census_cases.small_list()
    coords, ss, k, target, max_rounds = parts[1]
    _, begin, events = trace_oracle.pinned(coords, table, ss, k, target, max_rounds)
    with pytest.raises(ValueError, match="turn_bins"):
        rc.RollCensus.from_events(events, begin, ss, len(table), 1)
    with pytest.raises(ValueError, match="outside the table"):
        rc.RollCensus.from_events(events, begin, ss, 3, 8)
    with pytest.raises(ValueError, match="event_begin ends"):
        rc.RollCensus.from_events(events[:-1], begin, ss, len(table), 8)
    with pytest.raises(ValueError, match="do not merge"):
        rc.RollCensus.zeros(3, 8).merge(rc.RollCensus.zeros(3, 9))
    empty = rc.RollCensus.from_events(events[:0], np.zeros(2, np.int64), ss, len(table), 8)
    assert empty.equals(rc.RollCensus.zeros(len(table), 8))


def hand_made_census() -> rc.RollCensus:
    """One die: 60 rolls as [30 farkles, 20 fives, 10 ones] against the law's [40, 10, 10]; two dice: exactly 36 x the law; strategy 0
    with ten turns — four farkles, three turns of 300, three in the clamp bin (600 each) — strategy 1 without a turn."""
    census = rc.RollCensus.zeros(2, 8)
    census.roll_cells[0, 0, 0], census.roll_cells[0, 1, 1], census.roll_cells[0, 2, 1] = 30, 20, 10
    census.roll_cells[1] = rc.exact_cells()[1] * 36
    census.strategy_dice[0, 0] = (60, 30, 30)
    census.strategy_dice[0, 1] = (36 * 36, 36 * 16, int(census.roll_cells[1][:, 2].sum()))
    census.strategy_turns[0] = (10, 4, 3 * 300 + 3 * 600)
    census.turn_hist[0, 0], census.turn_hist[0, 6], census.turn_hist[0, 7] = 4, 3, 3
    return census


def test_roll_fit_on_a_hand_made_census():
    fit = rc.roll_fit(hand_made_census())
    assert fit["dice_count"].tolist() == [1, 2, 3, 4, 5, 6] and fit["cells"].tolist() == [3, 6, 12, 22, 35, 49]
    assert fit["dof"].tolist() == [2, 5, 11, 21, 34, 48] and fit["rolls"].tolist() == [60, 1296, 0, 0, 0, 0]
    one = fit.iloc[0]
    assert one["chi2"] == pytest.approx(100 / 40 + 100 / 10, rel=1e-12)                  # (30-40)^2/40 + (20-10)^2/10 + 0
    assert one["p_value"] == pytest.approx(math.exp(-12.5 / 2), rel=1e-9)               # chi2.sf with two degrees of freedom
    assert one["observed_farkle_probability"] == 0.5 and one["farkle_probability"] == 4 / 6
    assert one["observed_hot_dice_probability"] == 0.5 and one["hot_dice_probability"] == 2 / 6
    two = fit.iloc[1]
    assert two["chi2"] == 0.0 and two["p_value"] == 1.0 and two["observed_farkle_probability"] == two["farkle_probability"] == 16 / 36
    assert two["observed_hot_dice_probability"] == two["hot_dice_probability"] == 4 / 36  # 1-1, 1-5, 5-1, 5-5
    assert fit["chi2"].iloc[2:].isna().all() and fit["p_value"].iloc[2:].isna().all()
    assert "random" in rc.roll_fit.__doc__ and "not a test at a stated" in " ".join(rc.roll_fit.__doc__.split())
    observed = rc.observed_roll_distribution(hand_made_census())
    assert len(observed) == 127 and observed["observed_count"].iloc[:3].tolist() == [30, 20, 10]
    assert observed["expected_count"].iloc[:3].tolist() == [60 * (4 / 6), 60 * (1 / 6), 60 * (1 / 6)]
    assert observed["ordered_outcome_probability"].map(float.hex).tolist() == [r[7] for r in GOLDEN["distribution"]["rows"]]
    bad = hand_made_census()
    bad.roll_cells[0, 3, 1] = 1  # one die cannot score 150
    with pytest.raises(ValueError, match="outside the support"):
        rc.roll_fit(bad)


def test_strategy_turn_table_on_a_hand_made_census():
    frame = rc.strategy_turn_table(hand_made_census(), [11, 22])
    a, b = frame.iloc[0], frame.iloc[1]
    assert frame["strategy"].tolist() == [11, 22] and a["turns"] == 10 and a["farkle_turn_rate"] == 0.4 and a["mean_turn_score"] == 270.0
    assert a["rolls"] == 60 + 1296 and a["rolls_per_turn"] == 135.6 and a["farkle_rate_1_dice"] == 0.5 and a["farkle_rate_2_dice"] == 16 / 36
    assert math.isnan(a["farkle_rate_3_dice"]) and a["rolls_3_dice"] == 0
    assert a["p10_turn_score"] == 0.0 and a["median_turn_score"] == 300.0 and math.isnan(a["p90_turn_score"])  # p90 lies in the clamp bin
    assert b["turns"] == 0 and all(math.isnan(b[name]) for name in ("farkle_turn_rate", "mean_turn_score", "median_turn_score", "farkle_rate_1_dice"))
    with pytest.raises(ValueError, match="strategy ids"):
        rc.strategy_turn_table(hand_made_census(), [11])
