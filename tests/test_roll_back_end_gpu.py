"""The roll step's back end (fk_device.h: roll_back_end50, advance2_table50; the discard table's ready-made counter bits) through the
two-seat game kernel, bit-compared with the CPU oracle: a launch smaller than one block, a launch in which lanes take second tickets,
a table on which every game runs to the round limit, a batched H2H launch with a block that never completes, one listed game."""
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


def test_three_shuffles_rows_and_seat_statistics(eng, po, g64):
    """96 games: one full wave and one half-filled wave; every other resident wave never gets a ticket."""
    from oracle_engine_stub import seat_stats_from_rows

    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 3, want_rows=True)
    got = eng.tournament(g64, 2, 42, 0, 3, want_rows=True, want_seat_stats=True)
    assert "fk_play_kernel<" in eng.last_play_instance() and eng.last_play_instance().endswith(", 2>")  # a two-seat instance
    assert np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref["rows"], 2, 64, 32, 3))


def test_lanes_take_second_tickets(eng, po, g64):
    """416 000 games on at most 393 216 resident lanes (256 CUs x two 768-lane blocks): tallies only."""
    n_sh = 13_000
    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, n_sh, n_threads=16)
    got = eng.tournament(g64, 2, 42, 0, n_sh)
    assert eng.last_play_instance() == "fk_play_kernel<768, true, 6, 49152u, false, false, 2>"  # the benchmark's instance
    assert np.array_equal(got["tally"], ref["tally"])


def test_every_game_ends_at_the_round_limit(eng, po, g64):
    never = g64.copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    ref = po.tournament(never.view(po.STRATEGY_DTYPE), 2, 7, 0, 4, max_rounds=3, want_rows=True)
    got = eng.tournament(never, 2, 7, 0, 4, max_rounds=3, want_rows=True)
    assert int(ref["tally"][:, :, 3].sum()) == 4 * 64  # one safety-limit exposure per seat and shuffle
    assert np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()


def test_h2h_launch_with_a_block_that_never_completes(eng, po, g64):
    never = g64.copy()
    never["dice_threshold"], never["require_both"] = 0, 1
    pairs = np.stack([g64[[3, 40]], never[[0, 2]], g64[[17, 9]]])
    got = eng.h2h_blocks(pairs, 42, [5, 6, 7], [0, 1, 0], 150, 300, max_rounds=20)
    for b in range(3):
        want = po.h2h_block(pairs[b].view(po.STRATEGY_DTYPE), 42, 5 + b, [0, 1, 0][b], 150, 300, 300, max_rounds=20)
        assert np.array_equal(got[b], want), b
    assert int(got[1][1]) == 0 and int(got[1][2]) == 300  # nothing completed: every attempt ran to the round limit


def test_one_listed_game(eng, po, g64):
    from farkle_ii_amd.backend import COORD_DTYPE

    coords = np.zeros(1, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 10, 123, 2, 5
    seat = np.array([[12, 51]], dtype=np.int32)
    rows = eng.play_games(coords, g64, seat, 2)
    ref = po.play_games(coords.view(po.COORD_DTYPE), g64.view(po.STRATEGY_DTYPE), seat, 2)
    assert rows.tobytes() == ref.tobytes()
