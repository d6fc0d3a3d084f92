"""fk_trace_games on the device: its events byte for byte the events of tests/trace_oracle.py (the CPU oracle's game loop restated on
its own primitives, pinned by `row == the oracle's row`), its rows byte for byte the rows of the game kernels (Engine.play_games,
Engine.tournament) and of the oracle, and the reference's `watch_game` messages through the real engine.

No case for FK_ERR_ROLL_LIMIT: no coordinates and strategies are known that make a turn of 1 000 rolls (see
tests/test_roll_bookkeeping_gpu.py), so the fuse of the trace kernel is not reached on the device by this suite."""
from __future__ import annotations

import ctypes as C
import hashlib
import logging

import golden_util as gu
import numpy as np
import pyoracle as po
import pytest
import trace_oracle

pytestmark = pytest.mark.gpu

VECTORS = gu.load("watch_vectors.json")
WATCH = {case["seed"]: case for case in VECTORS["watch"]}


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


def _strats(tuples):
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    return gu.strategies_from_tuples(tuples, STRATEGY_DTYPE)


def mixed_table() -> np.ndarray:
    """Config 2's 64-strategy grid (every strategy with auto_hot_dice and run_up_score) + sixteen of its strategies with one or both
    flags cleared and the smart discards varied: every flag differs somewhere in a wave."""
    g64 = _strats(gu.load("grid_vectors.json")["g64"])
    extra = g64[::4].copy()
    for i in range(len(extra)):
        extra[i]["auto_hot_dice"] = i & 1
        extra[i]["run_up_score"] = (i >> 1) & 1
        if i & 4:
            extra[i]["smart_one"] = 0
        if i & 8:
            extra[i]["smart_one"] = extra[i]["smart_five"] = 0
        extra[i]["favor_score"] = (i >> 2) & 1
        extra[i]["strategy_id"] = 1000 + i
    return np.concatenate([g64, extra])


def assert_trace_equals_everything(eng, coords, table, ss, k, target=10_000, max_rounds=200):
    """The three equalities: events == the helper's, rows == the game kernels' == the oracle's; event_begin[-1] == sum of rolls."""
    want_rows, want_begin, want_events = trace_oracle.pinned(coords, table, ss, k, target, max_rounds)
    rows, begin, events = eng.trace_games(coords, table, ss, k, target_score=target, max_rounds=max_rounds)
    assert np.array_equal(begin, want_begin)
    assert events.tobytes() == want_events.tobytes()
    assert rows.tobytes() == want_rows.tobytes()
    assert rows.tobytes() == eng.play_games(coords, table, ss, k, target_score=target, max_rounds=max_rounds).tobytes()
    assert int(begin[-1]) == int(rows["seats"]["rolls"].astype(np.int64).sum())
    return rows, begin, events


def test_200_two_seat_games_with_mixed_flags(eng):
    from farkle_ii_amd.backend import make_coords

    rs = np.random.default_rng(7)
    table = mixed_table()
    n = 200  # three full waves and a partial one
    coords = make_coords(103, 42, 2, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 32, size=n))
    ss = rs.integers(0, len(table), size=(n, 2))
    ss[:16, 1] = 64 + np.arange(16)  # each altered strategy is seated
    rows, begin, events = assert_trace_equals_everything(eng, coords, table, ss, 2)
    assert (events["flags"] & 8).any() and (events["discards"] != 0).any() and (events["flags"] & 5 == 5).any()


@pytest.mark.parametrize("k,n,target", [(1, 64, 2000), (3, 65, 2000), (5, 3, 1000), (13, 3, 1000), (128, 3, 1000)])
def test_seat_count_edges(eng, k, n, target):
    from farkle_ii_amd.backend import make_coords

    rs = np.random.default_rng(100 + k)
    table = mixed_table()
    coords = make_coords(103, 11, k, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 40, size=n))
    ss = np.stack([rs.permutation(len(table) if k <= len(table) else k)[:k] % len(table) for _ in range(n)])
    assert_trace_equals_everything(eng, coords, table, ss, k, target=target)


@pytest.fixture(scope="module")
def extremes():
    """The 1 727-roll safety-limit game of watch seed 253 between the ~45-roll games of seeds 47 and 6, in one wave."""
    from farkle_ii_amd.backend import make_coords
    from farkle_ii_amd.strategies import pack_strategies
    from farkle_ii_amd.watch_game import watch_strategies

    seeds = [47, 6, 47, 6, 253, 47, 6, 47, 6]
    table = pack_strategies([s for seed in (253, 47, 6) for s in watch_strategies(seed)])
    first = {253: 0, 47: 2, 6: 4}
    coords = make_coords(10, np.array(seeds, dtype=np.uint64), 2)
    ss = np.array([[first[s], first[s] + 1] for s in seeds])
    return coords, table, ss


@pytest.mark.parametrize("max_rounds", [200, 3, 0])
def test_length_extremes_in_one_launch(eng, extremes, max_rounds):
    coords, table, ss = extremes
    rows, begin, events = assert_trace_equals_everything(eng, coords, table, ss, 2, max_rounds=max_rounds)
    lengths = np.diff(begin)
    if max_rounds == 200:
        assert lengths[4] == 1727 and rows[4]["status"] == 1 and lengths[[0, 1]].tolist() == [lengths[2], lengths[3]] and lengths[:4].max() < 60
    if max_rounds == 0:  # every range is empty; the counting call (events = NULL) is the whole call
        assert not begin.any() and len(events) == 0 and (rows["status"] == 1).all() and not rows["seats"]["rolls"].any()


def _raw_call(eng, coords, table, ss, k, rows, begin, events, capacity, target=10_000, max_rounds=200):
    from farkle_ii_amd.backend import _p

    return eng._lib.fk_trace_games(eng._ctx, _p(coords), C.c_int64(len(coords)), _p(table), C.c_int32(len(table)), _p(ss), C.c_int32(k),
                                   C.c_int32(target), C.c_int32(max_rounds), _p(rows), _p(begin), _p(events), C.c_int64(capacity))


def test_capacity_convention(eng):
    from farkle_ii_amd.backend import COORD_DTYPE, EVENT_DTYPE, FK_ERR_ARG, make_coords, row_dtype

    table = mixed_table()
    n, k = 70, 2
    coords = np.ascontiguousarray(make_coords(103, 3, k, shuffle_index=np.arange(n), game_index=1), dtype=COORD_DTYPE)
    ss = np.ascontiguousarray((np.arange(n * k) * 7) % len(table), dtype=np.int32)
    want_rows, want_begin, want_events = trace_oracle.pinned(coords, table, ss, k, 2000)
    total = int(want_begin[-1])
    rows, begin = np.zeros(n, dtype=row_dtype(k)), np.full(n + 1, -1, dtype=np.int64)
    assert _raw_call(eng, coords, table, ss, k, rows, begin, None, 0, target=2000) == 0  # the counting call
    assert np.array_equal(begin, want_begin) and rows.tobytes() == want_rows.tobytes()
    buf = np.zeros(total + 1, dtype=EVENT_DTYPE)
    buf.view(np.uint8)[:] = 0xA5  # canary everywhere: nothing may be stored
    begin[:] = -1
    assert _raw_call(eng, coords, table, ss, k, rows, begin, buf, total - 1, target=2000) == FK_ERR_ARG
    assert str(total) in eng._lib.fk_last_error(eng._ctx).decode()
    assert (buf.view(np.uint8) == 0xA5).all() and np.array_equal(begin, want_begin)
    assert _raw_call(eng, coords, table, ss, k, rows, begin, buf, total, target=2000) == 0  # the same context, exact size
    assert buf[:total].tobytes() == want_events.tobytes() and (buf[total:].view(np.uint8) == 0xA5).all()
    # argument checks come before any device work
    for bad_k, bad_ss in ((129, ss), (k, np.full_like(ss, len(table)))):
        assert _raw_call(eng, coords, table, bad_ss, bad_k, rows, begin, None, 0) == FK_ERR_ARG
    assert _raw_call(eng, coords, table, ss, k, rows, None, None, 0) == FK_ERR_ARG


def _watch(eng, caplog, seed):
    from farkle_ii_amd.watch_game import watch_game

    caplog.clear()
    with caplog.at_level(logging.INFO, logger="farkle_ii_amd.watch_game"):
        watch_game(seed, engine=eng)
    return [r.getMessage() for r in caplog.records if r.name == "farkle_ii_amd.watch_game"]


def test_watch_game_logs_the_reference_messages(eng, caplog):
    digest = lambda messages: hashlib.sha256("\n".join(messages).encode()).hexdigest()  # noqa: E731
    for seed in (47, 6, 42, 12, 25):
        assert _watch(eng, caplog, seed) == WATCH[seed]["messages"], seed
    mine = _watch(eng, caplog, 7)
    assert (len(mine), digest(mine)) == (WATCH[7]["count"], WATCH[7]["sha256"])
    mine = _watch(eng, caplog, 253)
    assert mine[-1] == "Winner: None  score=None  rounds=200"
    assert (len(mine) - 1, digest(mine[:-1])) == (WATCH[253]["count"], WATCH[253]["sha256"])


@pytest.mark.parametrize("case", VECTORS["scripted"], ids=lambda c: c["name"])
def test_scripted_flag_games(eng, case):
    from farkle_ii_amd.backend import make_coords
    from farkle_ii_amd.watch_game import render_rolls

    table = _strats(case["strategies"])
    coords = make_coords(case["purpose"], case["root_seed"], case["k"], shuffle_index=case["shuffle"], game_index=case["game"])
    rows, begin, events = assert_trace_equals_everything(eng, coords, table, np.arange(case["k"])[None, :], case["k"], case["target"],
                                                         case["max_rounds"])
    assert render_rolls(events) == case["messages"]


def test_replay_of_tournament_rows(eng):
    from farkle_ii_amd import trace

    table = _strats(gu.load("grid_vectors.json")["g64"])
    for shuffle, game in ((0, 0), (5, 15), (312_499, 7)):
        want = eng.tournament(table, 4, 42, shuffle, shuffle + 1, want_rows=True)["rows"][game]
        row, events, seats = trace.trace_tournament_game(eng, table, 42, 4, shuffle, game)
        assert row.tobytes() == want.tobytes() and seats.tolist() == want["seats"]["strategy"].tolist()
        trace.check(events, [0, len(events)], np.array([row]), seats, 4)
        assert row.tobytes() == po.play_game(po.coord(103, 42, 4, shuffle, game_index=game), table.view(po.STRATEGY_DTYPE), seats)[0].tobytes()
