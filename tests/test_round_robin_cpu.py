"""The host side of the round robin (farkle_ii_amd/round_robin.py) on synthetic block states, no engine: the summary against a literal
loop over blocks, the three frames (columns, order, null rates at zero denominators), additivity over roots and adjacent pair ranges,
and every refusal of the Python layer."""
from __future__ import annotations

from itertools import combinations

import numpy as np
import pytest

from farkle_ii_amd import round_robin as rr

TARGET, MAX_ATTEMPTS = 9, 15
IDS = np.array([3, 7, 8, 20, 21, 40, 77], dtype=np.int64)  # sorted strategy ids of a 7-row table: 21 pairs


def _states(n_pairs: int, seed: int) -> np.ndarray:
    """Consistent block states: completed + safety == attempted, wins sum to completed; complete, unresolved and zero-completed blocks."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n_pairs, 2, 5), dtype=np.uint32)
    for p in range(n_pairs):
        for o in range(2):
            kind = rng.integers(0, 4)
            if kind == 0:    # complete at once
                completed, safety = TARGET, 0
            elif kind == 1:  # complete with replacements
                completed, safety = TARGET, int(rng.integers(1, MAX_ATTEMPTS - TARGET + 1))
            elif kind == 2:  # unresolved with some games
                completed = int(rng.integers(1, TARGET))
                safety = MAX_ATTEMPTS - completed
            else:            # nothing completed
                completed, safety = 0, MAX_ATTEMPTS
            w1 = int(rng.integers(0, completed + 1))
            st[p, o] = (completed + safety, completed, safety, w1, completed - w1)
    st[0] = [(MAX_ATTEMPTS, 0, MAX_ATTEMPTS, 0, 0)] * 2  # a pair without a single completed game: every rate of it is null
    return st


def _loop_summary(n: int, states: np.ndarray, begin: int) -> np.ndarray:
    pairs = list(combinations(range(n), 2))
    out = np.zeros((n, 8), dtype=np.int64)
    wins = {}
    for row in range(len(states)):
        i, j = pairs[begin + row]
        wins[row] = {i: 0, j: 0}
        for order in (0, 1):
            attempted, completed, safety, w1, w2 = (int(v) for v in states[row, order])
            seat1, seat2 = (i, j) if order == 0 else (j, i)
            for s in (i, j):
                out[s, 2] += completed
                out[s, 3] += safety
            out[seat1, 4] += w1
            out[seat2, 4] += w2
            out[seat1, 5] += completed
            out[seat1, 6] += w1
            wins[row][seat1] += w1
            wins[row][seat2] += w2
        resolved = all(int(states[row, o, 1]) >= TARGET for o in (0, 1))
        for s, other in ((i, j), (j, i)):
            out[s, 0] += 1
            out[s, 1] += resolved
            out[s, 7] += resolved and wins[row][s] > wins[row][other]
    return out


def test_summary_against_a_literal_loop_over_blocks():
    n = len(IDS)
    st = _states(rr.pair_count(n), 1)
    got = rr.summary_from_states(n, st, TARGET)
    assert got.dtype == np.int64 and got.shape == (n, 8)
    assert np.array_equal(got, _loop_summary(n, st, 0))
    assert got[:, 0].tolist() == [n - 1] * n and 0 < got[:, 1].sum() < got[:, 0].sum() and got[:, 7].sum() > 0
    part = rr.summary_from_states(n, st[5:13], TARGET, 5, 13)
    assert np.array_equal(part, _loop_summary(n, st[5:13], 5))
    acc = rr.summary_from_states(n, st[:5], TARGET, 0, 5)
    assert rr.summary_from_states(n, st[5:], TARGET, 5, None, summary=acc) is acc and np.array_equal(acc, got)


def test_frames_columns_order_and_null_rates():
    n = len(IDS)
    roots = [11, 2**63 + 5]
    states = [_states(rr.pair_count(n), 1), _states(rr.pair_count(n), 2)]
    blocks = rr.blocks_frame(IDS, roots, states, TARGET, MAX_ATTEMPTS)
    assert tuple(blocks.columns) == rr.BLOCK_SCHEDULE_COLUMNS + rr.BLOCK_PROGRESS_COLUMNS
    assert tuple(blocks.columns[:11]) == ("pair_id", "strategy_a", "strategy_b", "root_seed", "root_index", "order", "order_label",
                                          "seat1_strategy", "seat2_strategy", "n_completed_required", "max_attempts")
    want_rows = []
    for pid, (i, j) in enumerate(combinations(range(n), 2)):  # _schedule_frame's loop nest: pair, root, order
        for r, root in enumerate(roots):
            for order in (0, 1):
                a, c, s, w1, w2 = (int(v) for v in states[r][pid, order])
                status = "complete" if c >= TARGET else "unresolved_nonviable" if a >= MAX_ATTEMPTS else "partial_resumable"
                want_rows.append((pid, IDS[i], IDS[j], root, r, order, "a_b" if order == 0 else "b_a", IDS[i] if order == 0 else IDS[j],
                                  IDS[j] if order == 0 else IDS[i], TARGET, MAX_ATTEMPTS, a, c, s, w1, w2, w1 if order == 0 else w2,
                                  w2 if order == 0 else w1, max(0, a - TARGET), status))
    assert [tuple(row) for row in blocks.itertuples(index=False)] == want_rows
    assert blocks["root_seed"].dtype == np.uint64 and set(blocks["completion_status"]) == {"complete", "unresolved_nonviable"}

    pairs = rr.pairs_frame(IDS, roots, states, TARGET)
    assert tuple(pairs.columns) == ("pair_id", "strategy_a", "strategy_b", "games_completed", "wins_a", "wins_b", "a_win_rate_order0",
                                    "a_win_rate_order1", "seat_balanced_a_win_rate", "seat1_win_rate", "resolved")
    pooled = states[0].astype(np.int64) + states[1].astype(np.int64)
    for pid, (i, j) in enumerate(combinations(range(n), 2)):
        row = pairs.iloc[pid]
        a, b = pooled[pid, 0], pooled[pid, 1]
        assert (row.pair_id, row.strategy_a, row.strategy_b) == (pid, IDS[i], IDS[j])
        assert (row.games_completed, row.wins_a, row.wins_b) == (a[1] + b[1], a[3] + b[4], a[4] + b[3])
        r0 = a[3] / a[1] if a[1] else None
        r1 = b[4] / b[1] if b[1] else None
        for got, want in ((row.a_win_rate_order0, r0), (row.a_win_rate_order1, r1),
                          (row.seat_balanced_a_win_rate, None if r0 is None or r1 is None else 0.5 * (r0 + r1)),
                          (row.seat1_win_rate, (a[3] + b[3]) / (a[1] + b[1]) if a[1] + b[1] else None)):
            assert np.isnan(got) if want is None else got == want, (pid, got, want)
        assert bool(row.resolved) == all(int(st[pid, o, 1]) >= TARGET for st in states for o in (0, 1))
    assert pairs.iloc[0][["a_win_rate_order0", "a_win_rate_order1", "seat_balanced_a_win_rate", "seat1_win_rate"]].isna().all()

    summary = rr.summary_from_states(n, states[0], TARGET)
    rr.summary_from_states(n, states[1], TARGET, summary=summary)
    summary[2, 2:7] = 0  # a strategy without a completed game
    strategies = rr.strategies_frame(IDS, summary)
    assert tuple(strategies.columns) == ("strategy_id", "pairs", "pairs_resolved", "games_completed", "games_safety", "wins",
                                         "seat1_games_completed", "seat1_wins", "pairs_ahead", "win_rate", "seat1_win_rate")
    assert strategies["strategy_id"].tolist() == IDS.tolist()
    assert np.array_equal(strategies[list(rr.SUMMARY_COLS)].to_numpy(), summary)
    assert np.isnan(strategies["win_rate"][2]) and np.isnan(strategies["seat1_win_rate"][2])
    assert strategies["win_rate"][0] == summary[0, 4] / summary[0, 2] and strategies["seat1_win_rate"][0] == summary[0, 6] / summary[0, 5]
    import pyarrow as pa

    assert pa.Table.from_pandas(strategies, preserve_index=False)["win_rate"].null_count == 1  # null in the written table


def test_roots_and_adjacent_ranges_add_up_to_the_whole():
    n = len(IDS)
    total = rr.pair_count(n)
    roots = [11, 23]
    states = [_states(total, 3), _states(total, 4)]
    cut = 8
    whole = rr.blocks_frame(IDS, roots, states, TARGET, MAX_ATTEMPTS)
    import pandas as pd

    # two adjacent pair ranges concatenate to the whole, in every frame
    halves = [rr.blocks_frame(IDS, roots, [st[lo:hi] for st in states], TARGET, MAX_ATTEMPTS, lo, hi) for lo, hi in ((0, cut), (cut, total))]
    assert pd.concat(halves, ignore_index=True).equals(whole)
    pairs = rr.pairs_frame(IDS, roots, states, TARGET)
    halves = [rr.pairs_frame(IDS, roots, [st[lo:hi] for st in states], TARGET, lo, hi) for lo, hi in ((0, cut), (cut, total))]
    assert pd.concat(halves, ignore_index=True).equals(pairs)
    summary = sum(rr.summary_from_states(n, st[lo:hi], TARGET, lo, hi) for st in states for lo, hi in ((0, cut), (cut, total)))
    assert np.array_equal(summary, rr.summary_from_states(n, states[0], TARGET) + rr.summary_from_states(n, states[1], TARGET))
    # two roots: the blocks of each root are the whole's rows of that root; the pair counts add
    for r, root in enumerate(roots):
        one = rr.blocks_frame(IDS, [root], [states[r]], TARGET, MAX_ATTEMPTS)
        sub = whole[whole["root_index"] == r].reset_index(drop=True)
        assert one.drop(columns="root_index").equals(sub.drop(columns="root_index"))
    singles = [rr.pairs_frame(IDS, [root], [states[r]], TARGET) for r, root in enumerate(roots)]
    for column in ("games_completed", "wins_a", "wins_b"):
        assert np.array_equal(pairs[column], singles[0][column] + singles[1][column])
    assert np.array_equal(pairs["resolved"], singles[0]["resolved"] & singles[1]["resolved"])
    both = rr.strategies_frame(IDS, summary)
    parts = [rr.strategies_frame(IDS, rr.summary_from_states(n, st, TARGET)) for st in states]
    for column in rr.SUMMARY_COLS:
        assert np.array_equal(both[column], parts[0][column] + parts[1][column])


def test_every_refusal_of_the_python_layer(tmp_path):
    n = len(IDS)
    st = _states(rr.pair_count(n), 5)
    with pytest.raises(ValueError, match="negative size"):
        rr.pair_count(-1)
    with pytest.raises(ValueError, match="at least two strategies"):
        rr.pair_ids(1)
    with pytest.raises(ValueError, match=r"pair range \[5, 4\) is not inside the 21 pairs of 7 strategies"):
        rr.pair_ids(n, 5, 4)
    with pytest.raises(ValueError, match=r"pair range \[0, 22\)"):
        rr.summary_from_states(n, st, TARGET, 0, 22)
    with pytest.raises(ValueError, match=r"must have shape \(21, 2, 5\)"):
        rr.summary_from_states(n, st[:20], TARGET)
    with pytest.raises(ValueError, match="summary must be int64"):
        rr.summary_from_states(n, st, TARGET, summary=np.zeros((n, 8), dtype=np.int32))
    with pytest.raises(ValueError, match="strictly ascending"):
        rr.blocks_frame(IDS[::-1], [1], [st], TARGET, MAX_ATTEMPTS)
    with pytest.raises(ValueError, match="one state array per root"):
        rr.pairs_frame(IDS, [1, 2], [st], TARGET)
    with pytest.raises(ValueError, match="one state array per root"):
        rr.blocks_frame(IDS, [], [], TARGET, MAX_ATTEMPTS)
    with pytest.raises(ValueError, match=r"summary must have shape \(7, 8\)"):
        rr.strategies_frame(IDS, np.zeros((6, 8), dtype=np.int64))
    for bad in (0.99, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="head2head.max_attempt_multiplier must be finite and at least 1"):
            rr.max_attempts_for(10, bad)
    with pytest.raises(ValueError, match="--block-games must be at least 1"):
        rr.max_attempts_for(0)
    assert rr.max_attempts_for(2191) == 4382 and rr.max_attempts_for(7, 1.5) == 11 and rr.max_attempts_for(7, 1.0) == 7
    with pytest.raises(ValueError, match="--pairs takes BEGIN:END"):
        rr.parse_pair_range("3-5", n)
    with pytest.raises(ValueError, match=r"pair range \[3, 99\)"):
        rr.parse_pair_range("3:99", n)
    assert rr.parse_pair_range(None, n) == (0, 21) and rr.parse_pair_range("4:", n) == (4, 21) and rr.parse_pair_range(":6", n) == (0, 6)
    ids_file = tmp_path / "ids.txt"
    ids_file.write_text("7\n\nx9\n")
    with pytest.raises(ValueError, match="ids.txt:3: not a strategy id"):
        rr.read_strategy_ids(ids_file)

    class S:
        def __init__(self, sid):
            self.strategy_id = sid

    grid = [S(int(v)) for v in IDS[::-1]]
    assert [s.strategy_id for s in rr.select_strategies(grid, None)] == IDS.tolist()           # sorted by id
    assert [s.strategy_id for s in rr.select_strategies(grid, [40, 3, 21])] == [3, 21, 40]
    with pytest.raises(ValueError, match="at least two strategies, got 1"):
        rr.select_strategies(grid, [40])
    with pytest.raises(ValueError, match=r"not in the configuration's grid: \[5, 6\]"):
        rr.select_strategies(grid, [3, 6, 5, 7])
    with pytest.raises(ValueError, match=r"duplicate strategy ids in the id file: \[7\]"):
        rr.select_strategies(grid, [3, 7, 7])
