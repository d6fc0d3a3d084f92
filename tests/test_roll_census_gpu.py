"""fk_census_games / fk_tournament_run_census on the device.  Every comparison is exact integer equality:

* ``census_games`` against ``RollCensus.from_events(fk_trace_games(...))`` on the same list — the census is a pure function of the
  trace's event stream, and the trace's events are pinned byte for byte against the CPU oracle by tests/test_trace_gpu.py;
* ``census_games`` and ``tournament_census`` against the census of the CPU oracle's own events (tests/trace_oracle.py) — directly,
  so that the census kernel's restatement of the game loop does not rest on the trace kernel's alone;
* chunked against unchunked, a second call against the first (the tables are set, not added to);
* ``tournament_census`` against ``census_games`` on the replay coordinates of the same games (``trace.tournament_seats``), and its
  per-strategy rolls, farkles and turns against the sums the hot game kernels report for the same shuffles
  (``Engine.tournament(want_seat_stats=True)``).

No case for FK_ERR_ROLL_LIMIT: no coordinates and strategies are known that make a turn of 1 000 rolls (tests/test_trace_gpu.py,
tests/test_roll_bookkeeping_gpu.py), so the census kernel's fuse, like the trace kernel's, is not reached on the device by this suite.  ``test_errors_leave_the_context_usable`` covers what can be reached: the
argument errors of both entries, untouched tables after a failed call, and a successful call on the same context afterwards."""
from __future__ import annotations

import ctypes as C

import census_cases
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLES = ("roll_cells", "strategy_dice", "strategy_turns", "turn_hist")


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


def from_trace(eng, coords, table, ss, k, target=10_000, max_rounds=200, turn_bins=256):
    from farkle_ii_amd.roll_census import RollCensus

    _, begin, events = eng.trace_games(coords, table, ss, k, target_score=target, max_rounds=max_rounds)
    return RollCensus.from_events(events, begin, np.asarray(ss).reshape(len(coords), k), len(table), turn_bins)


def device_census(eng, coords, table, ss, k, target=10_000, max_rounds=200, turn_bins=256):
    from farkle_ii_amd.roll_census import RollCensus

    return RollCensus.from_engine(eng.census_games(coords, table, ss, k, target_score=target, max_rounds=max_rounds, turn_bins=turn_bins))


def assert_same(got, want, what=""):
    for name in TABLES:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype == np.int64, (what, name)
        assert np.array_equal(a, b), (what, name, int(np.abs(a - b).sum()))


@pytest.fixture(scope="module")
def list257():
    coords, table, ss = census_cases.two_seat_list(257)
    return coords, table, ss


@pytest.fixture(scope="module")
def want257(eng, list257):
    """The reference of the 257-game list, computed once: {turn_bins: census from the trace's events}."""
    coords, table, ss = list257
    return {bins: from_trace(eng, coords, table, ss, 2, turn_bins=bins) for bins in (8, 256)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("turn_bins", [8, 256])
def test_two_seat_lists_equal_the_census_of_the_trace(eng, list257, want257, n, turn_bins):
    coords, table, ss = list257
    want = want257[turn_bins] if n == 257 else from_trace(eng, coords[:n], table, ss[:n], 2, turn_bins=turn_bins)
    got = device_census(eng, coords[:n], table, ss[:n], 2, turn_bins=turn_bins)
    assert_same(got, want, n)
    assert got.roll_cells.sum() > 0 and got.outside_support() == 0
    assert np.array_equal(got.turn_hist.sum(axis=1), got.strategy_turns[:, 0])
    if n == 257 and turn_bins == 8:
        assert got.turn_hist[:, 7].sum() > 0  # the clamp bin is reached


@pytest.mark.parametrize("k,target", [(1, 10_000), (3, 10_000), (5, 10_000), (13, 2000), (128, 2000)])
def test_seat_counts_with_100_games_each(eng, k, target):
    from farkle_ii_amd.backend import make_coords

    rs = np.random.default_rng(100 + k)
    table = census_cases.mixed_table()
    n = 100
    coords = make_coords(103, 11, k, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 40, size=n), n=n)
    ss = np.stack([rs.permutation(len(table) if k <= len(table) else k)[:k] % len(table) for _ in range(n)])
    assert_same(device_census(eng, coords, table, ss, k, target), from_trace(eng, coords, table, ss, k, target), k)


@pytest.fixture(scope="module")
def extremes():
    """The 1 727-roll safety-limit game of watch seed 253 between the ~45-roll games of seeds 47 and 6, in one wave (the list of
    tests/test_trace_gpu.py)."""
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
def test_length_extremes_in_one_wave(eng, extremes, max_rounds):
    coords, table, ss = extremes
    got = device_census(eng, coords, table, ss, 2, max_rounds=max_rounds)
    assert_same(got, from_trace(eng, coords, table, ss, 2, max_rounds=max_rounds), max_rounds)
    if max_rounds == 200:
        assert int(got.strategy_dice[:2, :, 0].sum()) == 1727  # the long game's two strategies sit in no other game
    if max_rounds == 0:  # no game rolls: every table is zero
        assert not any(getattr(got, name).any() for name in TABLES)


def test_one_strategy_takes_every_atomic_on_one_row(eng, list257):
    coords, table, _ = list257
    one = table[70:71]  # an altered strategy: auto_hot_dice off
    ss = np.zeros((len(coords), 2), dtype=np.int32)
    got = device_census(eng, coords, one, ss, 2, turn_bins=8)
    assert_same(got, from_trace(eng, coords, one, ss, 2, turn_bins=8))
    assert got.strategy_dice.shape == (1, 6, 3) and int(got.strategy_dice[0, :, 0].sum()) == int(got.roll_cells.sum()) > 10_000


@pytest.mark.parametrize("chunk", [64, 100])
def test_chunked_calls_equal_the_unchunked_one(eng, list257, want257, chunk):
    coords, table, ss = list257
    eng.set_option("census_chunk_games", chunk)  # 64: four full chunks and a one-game tail; 100: two chunks and a 57-game tail
    try:
        got = device_census(eng, coords, table, ss, 2)
        launches = eng.timing()["play_launches"]
    finally:
        eng.set_option("census_chunk_games", 0)
    assert launches == -(-257 // chunk)
    assert_same(got, want257[256], chunk)
    device_census(eng, coords, table, ss, 2)
    assert eng.timing()["play_launches"] == 1


def test_repeated_calls_set_the_tables(eng, list257, want257):
    coords, table, ss = list257
    first = device_census(eng, coords, table, ss, 2)
    second = device_census(eng, coords, table, ss, 2)
    assert_same(second, first)
    assert_same(second, want257[256])
    small = device_census(eng, coords[:3], table, ss[:3], 2)  # a smaller call after a larger one: nothing of the larger one is left
    assert_same(small, from_trace(eng, coords[:3], table, ss[:3], 2))


def oracle_census(coords, table, ss, k, max_rounds=200, turn_bins=256):
    """The census of the CPU oracle's events for the list (each game's row pinned against the oracle's row)."""
    import trace_oracle
    from farkle_ii_amd.roll_census import RollCensus

    _, begin, events = trace_oracle.pinned(coords, table, ss, k, 10_000, max_rounds)
    return RollCensus.from_events(events, begin, np.asarray(ss).reshape(len(coords), k), len(table), turn_bins)


def test_lists_equal_the_census_of_the_oracles_events(eng, list257):
    """One full wave plus one lane of the two-seat list, with the clamp bin on the path, and a three-seat list of three games."""
    from farkle_ii_amd.backend import make_coords

    coords, table, ss = list257
    got = device_census(eng, coords[:65], table, ss[:65], 2, turn_bins=8)
    assert_same(got, oracle_census(coords[:65], table, ss[:65], 2, turn_bins=8), "two seats")
    assert got.turn_hist[:, 7].sum() > 0  # the clamp bin is reached
    coords3 = make_coords(103, 11, 3, shuffle_index=np.array([5, 6, 7]), game_index=np.array([0, 1, 2]), n=3)
    ss3 = np.array([[0, 65, 70], [79, 3, 66], [71, 72, 1]], dtype=np.int32)
    assert_same(device_census(eng, coords3, table, ss3, 3, turn_bins=8), oracle_census(coords3, table, ss3, 3, turn_bins=8), "three seats")


def test_tournament_census_equals_the_census_of_the_oracles_events(eng):
    """k = 2, S = 8, shuffles 1 ... 4, max_rounds = 3 for one game in the middle: the permutations, the rebuilt coordinates and the
    override search of the tournament instance against the oracle's events for the same games."""
    from census_engine_stub import tournament_game_list
    from farkle_ii_amd.backend import OVERRIDE_DTYPE
    from farkle_ii_amd.roll_census import RollCensus

    table = census_cases.mixed_table()[[0, 21, 42, 63, 65, 70, 75, 79]]
    k, S, begin, end = 2, 8, 1, 5
    gps = S // k
    ov = np.zeros(1, dtype=OVERRIDE_DTYPE)
    ov[0] = (42, 3, 1, k, 3)  # shuffle 3, game 1: three rounds
    coords, ss = tournament_game_list(S, k, 42, begin, end)
    hit = (3 - begin) * gps + 1
    rest = np.setdiff1d(np.arange(len(coords)), [hit])
    want = oracle_census(coords[rest], table, ss[rest], k).merge(oracle_census(coords[hit:hit + 1], table, ss[hit:hit + 1], k, max_rounds=3))
    got = RollCensus.from_engine(eng.tournament_census(table, k, 42, begin, end, overrides=ov))
    assert_same(got, want)
    assert not got.equals(oracle_census(coords, table, ss, k))  # the override shortened a game


def replay_list(root, k, shuffle_begin, shuffle_end, S):
    """The games of a tournament range as an explicit list, by trace.py's tournament replay: (coords, seat_strategy)."""
    from farkle_ii_amd import trace
    from farkle_ii_amd.backend import make_coords

    gps = S // k
    sh = np.repeat(np.arange(shuffle_begin, shuffle_end, dtype=np.uint64), gps)
    g = np.tile(np.arange(gps, dtype=np.uint64), shuffle_end - shuffle_begin)
    coords = make_coords(103, root, k, shuffle_index=sh, game_index=g, n=len(g))
    ss = np.stack([trace.tournament_seats(root, k, int(s), int(i), S) for s, i in zip(sh.tolist(), g.tolist())])
    return coords, ss


@pytest.mark.parametrize("k,S,begin,end,spb", [(2, 64, 3, 8, 2), (5, 80, 0, 3, None), (3, 78, 1, 4, 2)])
def test_tournament_census_equals_census_games_on_the_replay_list(eng, k, S, begin, end, spb):
    from farkle_ii_amd.roll_census import RollCensus

    table = census_cases.g64() if S == 64 else census_cases.mixed_table()[:S]
    coords, ss = replay_list(42, k, begin, end, S)
    got = RollCensus.from_engine(eng.tournament_census(table, k, 42, begin, end, shuffles_per_batch=spb))
    assert_same(got, device_census(eng, coords, table, ss, k), (k, S))
    assert int(got.strategy_turns[:, 0].min()) > 0  # every strategy is seated once per shuffle


def test_tournament_refuses_a_table_k_does_not_divide(eng):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    with pytest.raises(FarkleHipError) as err:
        eng.tournament_census(census_cases.mixed_table(), 3, 42, 0, 2)  # 80 strategies at three seats: as fk_tournament_run
    assert err.value.args[0] == FK_ERR_ARG or "must divide" in str(err.value)


def test_tournament_census_with_a_max_rounds_override_in_the_middle(eng):
    from farkle_ii_amd.backend import OVERRIDE_DTYPE
    from farkle_ii_amd.roll_census import RollCensus

    table = census_cases.g64()
    k, S, begin, end = 2, 64, 3, 8
    gps = S // k
    ov = np.zeros(2, dtype=OVERRIDE_DTYPE)
    ov[0] = (42, 5, 7, k, 1)   # shuffle 5, game 7: one round
    ov[1] = (42, 5, 7, 4, 0)   # another k: not this tournament's
    coords, ss = replay_list(42, k, begin, end, S)
    hit = (5 - begin) * gps + 7
    rest = np.setdiff1d(np.arange(len(coords)), [hit])
    want = device_census(eng, coords[rest], table, ss[rest], k).merge(device_census(eng, coords[hit:hit + 1], table, ss[hit:hit + 1], k, max_rounds=1))
    got = RollCensus.from_engine(eng.tournament_census(table, k, 42, begin, end, shuffles_per_batch=2, overrides=ov))
    assert_same(got, want)
    plain = RollCensus.from_engine(eng.tournament_census(table, k, 42, begin, end, shuffles_per_batch=2))
    assert not plain.equals(got)  # the override shortened a game
    # the same range in chunks of one shuffle
    eng.set_option("census_chunk_games", gps)
    try:
        chunked = RollCensus.from_engine(eng.tournament_census(table, k, 42, begin, end, shuffles_per_batch=2, overrides=ov))
        assert eng.timing()["play_launches"] == end - begin
    finally:
        eng.set_option("census_chunk_games", 0)
    assert_same(chunked, want)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_tournament_census_totals_equal_the_hot_kernels_sums(eng, k):
    from farkle_ii_amd.backend import SEAT_STAT_NAMES
    from farkle_ii_amd.roll_census import RollCensus

    table = census_cases.g64()
    census = RollCensus.from_engine(eng.tournament_census(table, k, 7, 0, 12, shuffles_per_batch=5))
    stats = eng.tournament(table, k, 7, 0, 12, shuffles_per_batch=5, want_seat_stats=True, want_seat_ratios=False)["seat_stats"].sum(axis=0)
    col = {name: i for i, name in enumerate(SEAT_STAT_NAMES)}
    assert np.array_equal(census.strategy_dice[:, :, 0].sum(axis=1), stats[:, col["rolls_sum"]])
    assert np.array_equal(census.strategy_dice[:, :, 1].sum(axis=1), stats[:, col["farkles_sum"]])
    assert np.array_equal(census.strategy_turns[:, 0], stats[:, col["n_turns_sum"]])
    assert np.array_equal(census.strategy_turns[:, 1], stats[:, col["farkles_sum"]])


def test_errors_leave_the_context_usable(eng, list257, want257):
    from farkle_ii_amd.backend import COORD_DTYPE, FK_ERR_ARG, STRATEGY_DTYPE, FarkleHipError, _Census, _census_tables, _p

    coords, table, ss = list257
    coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
    table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE)
    flat = np.ascontiguousarray(ss, dtype=np.int32).reshape(-1)

    def raw(census, k=2, seats=flat, max_rounds=200):
        return eng._lib.fk_census_games(eng._ctx, _p(coords), C.c_int64(len(coords)), _p(table), C.c_int32(len(table)), _p(seats), C.c_int32(k),
                                        C.c_int32(10_000), C.c_int32(max_rounds), C.byref(census))

    tables, census = _census_tables(len(table), 256)
    for t in tables.values():
        t[...] = -1  # canary: a failed call stores nothing
    assert raw(census, k=129) == FK_ERR_ARG and raw(census, seats=np.full_like(flat, len(table))) == FK_ERR_ARG
    assert raw(census, max_rounds=70_000) == FK_ERR_ARG and raw(census, k=3) == FK_ERR_ARG  # (coordinates of another k)
    for bins in (1, 4097):
        bad = _Census(bins, *(tables[name].ctypes.data for name in TABLES))
        assert raw(bad) == FK_ERR_ARG and "turn_bins" in eng._lib.fk_last_error(eng._ctx).decode()
    assert raw(_Census(256, None, None, None, None)) == FK_ERR_ARG
    assert all((t == -1).all() for t in tables.values())
    with pytest.raises(FarkleHipError):
        eng.tournament_census(table, 2, 42, 0, 2, turn_bins=1)
    assert raw(census) == 0  # the same context, the same tables: now set
    for name in TABLES:
        assert np.array_equal(tables[name], getattr(want257[256], name)), name
