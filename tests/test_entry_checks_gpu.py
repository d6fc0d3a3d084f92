"""The first error of every playing entry.  The entries share their argument checks (csrc/farkle_hip.hip: check_list_shape,
check_list_games, check_seating, check_range, ...), each keeping the order it had when it stated them itself: a call with two defects
must report the one that came first then.  The expected codes and messages below were written from the entries' source as it was
before the checks were shared, and this file passed against a library built from that source.

Every case fails in the argument checks, before any launch; after its bad calls an entry must return what it returned before them."""
from __future__ import annotations

import ctypes as C

import census_cases
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEATS = "games have at most 128 seats (a row names its winner's seat in an int8), got 129"
ROUNDS = "max_rounds must be in [0, 65535]"
COORD_K = "Player RNG coordinate k does not match the number of seated strategies"


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


def refused(eng, rc, message):
    from farkle_ii_amd.backend import FK_ERR_ARG

    assert rc == FK_ERR_ARG, (rc, message)
    assert eng._lib.fk_last_error(eng._ctx).decode() == message


def i32(v):
    return C.c_int32(v)


def u64(v):
    return C.c_uint64(v)


def test_tournament_run(eng):
    from farkle_ii_amd.backend import STRATEGY_DTYPE, _p

    g64 = np.ascontiguousarray(census_cases.g64(), dtype=STRATEGY_DTYPE)
    tally = np.zeros((4, 65536, 8), dtype=np.int64)  # (room for every table below, whatever the tally's columns)

    def run(table=g64, S=None, k=2, begin=0, end=2, spb=2, target=10_000, max_rounds=200, ov=None, n_ov=0, out=tally):
        return eng._lib.fk_tournament_run(eng._ctx, _p(table), i32(len(table) if S is None else S), i32(k), u64(42), u64(begin), u64(end),
                                          C.c_uint32(spb), i32(target), i32(max_rounds), _p(ov), i32(n_ov), _p(out), None, None)

    before = eng.tournament(g64, 2, 42, 0, 2)["tally"].copy()
    refused(eng, run(out=None, k=3), "strategies and tally are required")
    refused(eng, run(k=3, max_rounds=70_000), "n_players must divide 64")
    refused(eng, run(k=0, begin=5, end=1), "n_players must divide 64")
    refused(eng, run(table=np.resize(g64, 258), k=129, max_rounds=-1), SEATS)
    refused(eng, run(table=np.resize(g64, 65536), max_rounds=70_000), "S=65536 exceeds 65535 strategies")
    refused(eng, run(max_rounds=70_000, begin=5, end=1), ROUNDS)
    refused(eng, run(spb=0, n_ov=-1), "bad shuffle range / batch size")
    refused(eng, run(n_ov=1, ov=None, target=10**9), "bad override list")
    assert np.array_equal(eng.tournament(g64, 2, 42, 0, 2)["tally"], before)


def test_tournament_run_census(eng):
    from farkle_ii_amd.backend import STRATEGY_DTYPE, _Census, _census_tables, _p

    g64 = np.ascontiguousarray(census_cases.g64(), dtype=STRATEGY_DTYPE)
    tables, good = _census_tables(64, 256)
    narrow = _Census(1, *(tables[name].ctypes.data for name in ("roll_cells", "strategy_dice", "strategy_turns", "turn_hist")))

    def run(table=g64, k=2, begin=0, end=2, spb=2, max_rounds=200, n_ov=0, out=good):
        return eng._lib.fk_tournament_run_census(eng._ctx, _p(table), i32(64), i32(k), u64(42), u64(begin), u64(end), C.c_uint32(spb), i32(10_000),
                                                 i32(max_rounds), None, i32(n_ov), C.byref(out) if out is not None else None)

    before = {name: t.copy() for name, t in eng.tournament_census(g64, 2, 42, 0, 2).items()}
    refused(eng, run(table=None, k=3), "strategies are required")
    refused(eng, run(k=3, max_rounds=70_000), "n_players must divide 64")
    refused(eng, run(max_rounds=70_000, out=narrow), ROUNDS)
    refused(eng, run(begin=5, end=1, out=None), "bad shuffle range / batch size")
    refused(eng, run(n_ov=-1, out=narrow), "bad override list")
    broken = g64.copy()
    broken["smart_one"][5], broken["smart_five"][5] = 1, 0
    refused(eng, run(out=narrow, table=broken), "turn_bins must be in [2, 4096], got 1")
    refused(eng, run(table=broken), "strategy 5: smart_one requires smart_five")
    after = eng.tournament_census(g64, 2, 42, 0, 2)
    assert all(np.array_equal(after[name], before[name]) for name in before)


@pytest.fixture(scope="module")
def games():
    """Five two-seat games, and their defects: a seat's strategy out of range, coordinates of another k and of a named seat."""
    from farkle_ii_amd.backend import COORD_DTYPE, STRATEGY_DTYPE

    coords, table, ss = census_cases.two_seat_list(5)
    coords = np.ascontiguousarray(coords, dtype=COORD_DTYPE)
    table = np.ascontiguousarray(table, dtype=STRATEGY_DTYPE)
    flat = np.ascontiguousarray(ss, dtype=np.int32).reshape(-1)
    bad_seat = flat.copy()
    bad_seat[3] = len(table)
    other_k = coords.copy()
    other_k["k"][1] = 3
    other_k["seat_index"][0] = 1  # (an earlier game, a later check: the coordinates are checked game by game)
    both = coords.copy()
    both["k"][0] = 3
    both["seat_index"][0] = 1
    return coords, table, flat, bad_seat, other_k, both


def test_play_games(eng, games):
    from farkle_ii_amd.backend import _p, row_dtype

    coords, table, flat, bad_seat, other_k, both = games
    rows = np.zeros(5, dtype=row_dtype(2))

    def run(co=coords, n=5, seats=flat, k=2, max_rounds=200, out=rows):
        return eng._lib.fk_play_games(eng._ctx, _p(co), C.c_int64(n), _p(table), i32(len(table)), _p(seats), i32(k), i32(10_000), i32(max_rounds),
                                      _p(out))

    before = eng.play_games(coords, table, flat, 2).tobytes()
    refused(eng, run(out=None, k=0), "coords, table, seat_strategy, rows are required")
    refused(eng, run(k=0, max_rounds=70_000), "bad k / S / n_games")
    refused(eng, run(n=-1, k=129), "bad k / S / n_games")
    refused(eng, run(k=129, max_rounds=70_000, seats=np.resize(flat, 5 * 129)), SEATS)
    refused(eng, run(max_rounds=-1, seats=bad_seat), ROUNDS)
    refused(eng, run(seats=bad_seat, co=other_k), "seat_strategy[3] out of range")
    refused(eng, run(co=other_k), "game coordinates carry seat_index 0 (seats are implied)")
    refused(eng, run(co=both), COORD_K)
    assert eng.play_games(coords, table, flat, 2).tobytes() == before


def test_trace_games(eng, games):
    from farkle_ii_amd.backend import EVENT_DTYPE, _p, row_dtype

    coords, table, flat, bad_seat, other_k, both = games
    rows, begin, events = np.zeros(5, dtype=row_dtype(2)), np.zeros(6, dtype=np.int64), np.zeros(8, dtype=EVENT_DTYPE)

    def run(co=coords, n=5, seats=flat, k=2, max_rounds=200, out=begin, ev=None, capacity=0):
        return eng._lib.fk_trace_games(eng._ctx, _p(co), C.c_int64(n), _p(table), i32(len(table)), _p(seats), i32(k), i32(10_000), i32(max_rounds),
                                       _p(rows), _p(out), _p(ev), C.c_int64(capacity))

    before = [a.tobytes() for a in eng.trace_games(coords, table, flat, 2)]
    refused(eng, run(out=None, k=0), "coords, table, seat_strategy, rows, event_begin are required")
    refused(eng, run(n=0x7FFFFFFF, k=1, max_rounds=70_000), "bad k / S / n_games")  # (one more game than the scan's int can count)
    refused(eng, run(k=129, max_rounds=70_000, seats=np.resize(flat, 5 * 129)), SEATS)
    refused(eng, run(max_rounds=70_000, ev=events, capacity=-1), ROUNDS)
    refused(eng, run(ev=events, capacity=-1, seats=bad_seat), "event_capacity must not be negative")
    refused(eng, run(seats=bad_seat, co=both), "seat_strategy[3] out of range")
    refused(eng, run(co=both, ev=events, capacity=1), COORD_K)
    assert [a.tobytes() for a in eng.trace_games(coords, table, flat, 2)] == before


def test_census_games(eng, games):
    from farkle_ii_amd.backend import _Census, _census_tables, _p

    coords, table, flat, bad_seat, other_k, both = games
    tables, good = _census_tables(len(table), 256)
    narrow = _Census(1, *(tables[name].ctypes.data for name in ("roll_cells", "strategy_dice", "strategy_turns", "turn_hist")))

    def run(co=coords, n=5, seats=flat, k=2, max_rounds=200, out=good):
        return eng._lib.fk_census_games(eng._ctx, _p(co), C.c_int64(n), _p(table), i32(len(table)), _p(seats), i32(k), i32(10_000), i32(max_rounds),
                                        C.byref(out))

    before = {name: t.copy() for name, t in eng.census_games(coords, table, flat, 2).items()}
    refused(eng, run(co=None, k=0), "coords, table, seat_strategy are required")
    refused(eng, run(n=0x7FFFFFFF, k=1, out=narrow), "bad k / S / n_games")
    refused(eng, run(k=129, out=narrow, seats=np.resize(flat, 5 * 129)), SEATS)
    refused(eng, run(max_rounds=70_000, out=narrow), ROUNDS)
    refused(eng, run(out=narrow, seats=bad_seat), "turn_bins must be in [2, 4096], got 1")
    refused(eng, run(seats=bad_seat, co=other_k), "seat_strategy[3] out of range")
    refused(eng, run(co=both), COORD_K)
    after = eng.census_games(coords, table, flat, 2)
    assert all(np.array_equal(after[name], before[name]) for name in before)


def test_h2h_run_blocks(eng):
    from farkle_ii_amd.backend import H2H_BLOCK_DTYPE, STRATEGY_DTYPE, _p

    g64 = np.ascontiguousarray(census_cases.g64(), dtype=STRATEGY_DTYPE)
    blocks = np.zeros(2, dtype=H2H_BLOCK_DTYPE)
    blocks["seats"] = np.stack([g64[[3, 40]], g64[[17, 9]]])
    blocks["pair_id"] = [5, 6]
    blocks["target"] = 20
    blocks["max_attempts"] = 40

    def run(b=blocks, n=2, max_rounds=200, n_ov=0):
        b = None if b is None else b.copy()  # (a call advances its blocks in place)
        return eng._lib.fk_h2h_run_blocks(eng._ctx, _p(b), C.c_int64(n), u64(42), u64(40), i32(10_000), i32(max_rounds), None, i32(n_ov))

    def good():
        return eng.h2h_blocks(blocks["seats"], 42, [5, 6], [0, 0], 20, 40)

    before = good()
    bad_order, bad_state = blocks.copy(), blocks.copy()
    bad_order["order"][0] = 2
    bad_order["state"][0] = [3, 1, 1, 1, 0]  # attempted 3, completed 1 + safety 1
    bad_state["state"][0] = [3, 1, 1, 1, 0]
    bad_state["order"][1] = 2
    refused(eng, run(b=None, max_rounds=70_000), "blocks are required (at most 2^22 per call)")
    refused(eng, run(n=(1 << 22) + 1, n_ov=-1), "blocks are required (at most 2^22 per call)")
    refused(eng, run(max_rounds=70_000, n_ov=-1), ROUNDS)
    refused(eng, run(n_ov=1, b=bad_order), "bad override list")
    refused(eng, run(b=bad_order), "block 0: order must be 0 or 1")
    refused(eng, run(b=bad_state), "block 0: inconsistent block state")
    assert np.array_equal(good(), before)


def test_h2h_round_robin(eng):
    from farkle_ii_amd.backend import STRATEGY_DTYPE, _p

    table = np.ascontiguousarray(census_cases.g64()[[3, 40, 17, 9]], dtype=STRATEGY_DTYPE)
    states = np.zeros((6, 2, 5), dtype=np.uint32)

    def run(t=table, n=4, begin=0, end=6, target=5, max_attempts=10, target_score=10_000, max_rounds=200, out=states):
        return eng._lib.fk_h2h_round_robin(eng._ctx, _p(t), i32(n), u64(42), u64(begin), u64(end), u64(target), u64(max_attempts), i32(target_score),
                                           i32(max_rounds), _p(out), None)

    before = eng.h2h_round_robin(table, 42, 5, 10)[0].copy()
    refused(eng, run(t=None, n=1), "the strategy table is required")
    refused(eng, run(n=1, max_rounds=70_000), "a round robin needs at least two strategies, got 1")
    refused(eng, run(end=99, target=0), "pair range [0, 99) is not inside the 6 pairs of 4 strategies")
    refused(eng, run(target=0, max_rounds=70_000), "target must be in [1, max_attempts] and max_attempts at most 2^31 - 1")
    refused(eng, run(max_attempts=1 << 31, target_score=10**9), "target must be in [1, max_attempts] and max_attempts at most 2^31 - 1")
    refused(eng, run(max_rounds=70_000, target_score=10**9), ROUNDS)
    refused(eng, run(max_rounds=-1, out=None), ROUNDS)
    assert np.array_equal(eng.h2h_round_robin(table, 42, 5, 10)[0], before)
