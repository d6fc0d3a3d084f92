"""The roll loop's per-trip bookkeeping (round 9) through the game kernels, bit-compared with the CPU oracle: the carried LDS address of
the turn owner's record and the xor-toggled increment address of the two-seat instances (fk_kernels.h: own_rec, own_inc_at; `seat` is
read back from the address where a game ends), the dice key accumulated as a byte offset (fk_device.h: roll_key_fast) and the discard
table's wide entries (discard_lut_entry32, roll_back_end50w), in every instance family that takes them: two seats with the LDS tally,
with rows and all-seat statistics, with flags that differ between the seats, the H2H block instance, three seats, and the forced-detour
build, in which the byte-offset key of the fast path and the plain key of the sequential path meet in every game.
(FK_ERR_ROLL_LIMIT is not reached on the device by any strategy pair the suite knows — a turn of 1 000 rolls needs hundreds of hot-dice
rolls in a row — so the limits themselves are covered on the host: tests/test_roll_guards_host.py.)"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle

    return pyoracle


@pytest.fixture(scope="module")
def g64():
    """The benchmark's 64-strategy grid: require_both and favor_score vary, the other flags are the same for the whole table."""
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies

    strategies, _ = generate_strategy_grid(
        score_thresholds=[250, 300, 350, 400], dice_thresholds=[0, 1, 2, 3], smart_five_opts=[True], smart_one_opts=[True],
        consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[True])
    table = pack_strategies(strategies)
    assert len(table) == 64
    return table


@pytest.fixture(scope="module")
def ref40(po, g64):
    """1 280 two-seat games, root seed 42: computed once, shared by the product build's and the detour build's tests."""
    return po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 40, want_rows=True, n_threads=8)


def _mixed16(g64):
    """16 strategies in which require_both, smart_one, auto_hot_dice and run_up_score each take both values (one per bit of the row
    number), so that the two seats of a game differ in every one of them in some game of every shuffle."""
    t = g64[[0, 5, 10, 15, 16, 21, 26, 31, 32, 37, 42, 47, 48, 53, 58, 63]].copy()
    i = np.arange(16)
    t["require_both"], t["smart_one"], t["auto_hot_dice"], t["run_up_score"] = i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1
    t["strategy_id"] = i
    return t


def test_tournament_tally(eng, po, g64, ref40):
    got = eng.tournament(g64, 2, 42, 0, 40)
    assert eng.last_play_instance() == "fk_play_kernel<768, true, 6, 49152u, false, false, 2>"  # the benchmark's instance
    assert np.array_equal(got["tally"][0], ref40["tally"].sum(axis=0))


def test_tournament_rows_and_seat_statistics(eng, po, g64, ref40):
    """finish_game reads both seats' records by seat number after the owner's address has been toggled an odd (seat 1 ends the game)
    and an even (seat 0 ends it) number of times: the winner's counters, the rows of both seats, every seat's statistics."""
    from oracle_engine_stub import seat_stats_from_rows

    got = eng.tournament(g64, 2, 42, 0, 40, want_rows=True, want_seat_stats=True)
    assert eng.last_play_instance().endswith(", 2>")
    assert np.array_equal(got["tally"], ref40["tally"])
    assert got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref40["rows"], 2, 64, 32, 40))


def test_flags_that_differ_between_the_seats(eng, po, g64):
    table = _mixed16(g64)
    for name in ("require_both", "smart_one", "auto_hot_dice", "run_up_score"):
        assert set(table[name]) == {0, 1}
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), 2, 42, 0, 64, want_rows=True, n_threads=8)
    got = eng.tournament(table, 2, 42, 0, 64, want_rows=True)
    assert eng.last_play_instance().endswith(", 2>")
    assert np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()
    counts = eng.tournament(table, 2, 42, 0, 64)  # tallies in LDS
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))


def test_h2h_block_instance(eng, po, g64):
    """One block of 2 000 target games: the strategy index comes from the lane's block, the owner's record from the carried address."""
    seats = g64[[3, 40]]
    got = eng.h2h(seats, 42, 5, 0, 2000, 4000, 10**6)
    assert eng.last_play_instance().endswith("true, 2>")  # BLK, two seats
    assert np.array_equal(got, po.h2h_block(seats.view(po.STRATEGY_DTYPE), 42, 5, 0, 2000, 4000, 10**6))


def test_three_seats(eng, po, g64):
    """The generic instance (seat-number addressing, `advance`): the key convention, the wide discard entries and the increments."""
    table = _mixed16(g64)[:12]
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), 3, 42, 0, 32, want_rows=True, n_threads=8)
    got = eng.tournament(table, 3, 42, 0, 32, want_rows=True)
    instance = eng.last_play_instance()
    assert instance.startswith("fk_play_kernel<") and instance.endswith(", 0>")
    assert np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()


def test_forced_detours(po, g64, ref40):
    """libfarkle_hip_detour.so (-DFK_FORCE_DETOUR=4): every fourth roll is replayed by roll_counts_sequential, which returns the plain
    key; the roll step turns it into the byte offset the fast path returns."""
    from farkle_ii_amd import backend

    backend.build_library(variant="detour")  # prebuilt by __graft_entry__.build()
    detour = backend.Engine(0, variant="detour")
    try:
        got = detour.tournament(g64, 2, 42, 0, 40, want_rows=True)
        counts = detour.tournament(g64, 2, 42, 0, 40)
    finally:
        detour.close()
    assert np.array_equal(got["tally"], ref40["tally"])
    assert got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(counts["tally"][0], ref40["tally"].sum(axis=0))


def test_listed_games_of_a_pair_that_never_banks_end_at_the_round_limit(eng, po, g64):
    """Two-seat game list (play_games) with a round limit of its own: nobody banks, every game ends at max_rounds with the turn back at
    seat 1's record — the end state from which finish_game derives the owner without a carried seat number."""
    from farkle_ii_amd.backend import COORD_DTYPE

    never = g64.copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    coords = np.zeros(6, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 10, 123, 2, np.arange(6)
    seat = np.array([[12, 51], [0, 63], [7, 7], [33, 2], [5, 60], [18, 41]], dtype=np.int32)
    for max_rounds in (1, 4):
        rows = eng.play_games(coords, never, seat, 2, max_rounds=max_rounds)
        ref = po.play_games(coords.view(po.COORD_DTYPE), never.view(po.STRATEGY_DTYPE), seat, 2, max_rounds=max_rounds)
        assert rows.tobytes() == ref.tobytes(), max_rounds
