"""The shortened flat hand-over of the two-seat game kernel (round 11), bit-compared with the CPU oracle at the smallest shapes at which
it can go wrong.  What changed in fk_kernels.h: a served lane's ticket is formed by selects and `init_game2` sits in one region; a
hand-over falls through into the roll loop instead of going round the outer loop; `finish_game2` reads both score words, selects the
winner's record address and loads that record alone; eight of the ten sums of squares are 32-bit products (fk_device.h:
`finish2_square`).  Covered: fewer games than lanes, a partial ticket chunk and an exhausted pool (1, 2, 3, 5 shuffles of 32 games against
chunks of 64 tickets) under thresholds 1, 8 and 64; game lists around the wave size; games that end at the round limit; a call in which
no round is played (a hand-over that deals ended games, then falls into the roll loop with nobody playing); every output kind the flat
path writes (LDS tally, `rec0`, `recs`, state out); the three strategy-flag forms; and option `flat_handover` 0 against 1.  A mistake
in this code shows as a hang: run this file under a time limit of its own."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESHOLDS = (1, 8, 64)


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.set_option("batch_threshold", 0)
    e.set_option("flat_handover", 1)
    e.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle

    return pyoracle


@pytest.fixture(scope="module")
def g64():
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies

    strategies, _ = generate_strategy_grid(
        score_thresholds=[250, 300, 350, 400], dice_thresholds=[0, 1, 2, 3], smart_five_opts=[True], smart_one_opts=[True],
        consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[True])
    table = pack_strategies(strategies)
    assert len(table) == 64
    return table


@pytest.fixture(scope="module")
def ref5(po, g64):
    """160 two-seat games (five shuffles), rows and per-shuffle tallies, computed once: the smaller cases are its prefixes."""
    return po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 5, shuffles_per_batch=1, want_rows=True, n_threads=8)


def _never_banking(g64):
    never = g64.copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    return never


def _with_threshold(eng, thr, call):
    try:
        eng.set_option("batch_threshold", thr)
        return call()
    finally:
        eng.set_option("batch_threshold", 0)


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("n_sh", [1, 2, 3, 5])
def test_pool_edges_under_every_threshold(eng, g64, ref5, n_sh, thr):
    """32, 64, 96 and 160 games: the LDS tally of a counts-only call (sums and sums of squares of the ten metrics), then the state store
    and the result records of a call with rows, one shuffle per batch."""
    counts = _with_threshold(eng, thr, lambda: eng.tournament(g64, 2, 42, 0, n_sh))
    assert eng.last_play_instance().endswith(", 2>")
    assert np.array_equal(counts["tally"][0], ref5["tally"][:n_sh].sum(axis=0))
    got = _with_threshold(eng, thr, lambda: eng.tournament(g64, 2, 42, 0, n_sh, shuffles_per_batch=1, want_rows=True))
    assert np.array_equal(got["tally"], ref5["tally"][:n_sh])
    assert got["rows"].tobytes() == ref5["rows"][:32 * n_sh].tobytes()


def test_every_output_kind(eng, g64, ref5):
    from oracle_engine_stub import seat_stats_from_rows

    counts = eng.tournament(g64, 2, 42, 0, 5)  # one batch, counts only: the LDS tally
    assert eng.timing()["play_lds_bytes"] > 2 * 768 * 40
    assert np.array_equal(counts["tally"][0], ref5["tally"].sum(axis=0))
    batches = eng.tournament(g64, 2, 42, 0, 5, shuffles_per_batch=1)  # several batches, counts only: rec0 instead of the LDS tally
    assert eng.timing()["play_lds_bytes"] == 2 * 768 * 40
    assert np.array_equal(batches["tally"], ref5["tally"])
    got = eng.tournament(g64, 2, 42, 0, 5, shuffles_per_batch=1, want_rows=True, want_seat_stats=True)  # state out + result records
    assert np.array_equal(got["tally"], ref5["tally"]) and got["rows"].tobytes() == ref5["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref5["rows"], 2, 64, 32, 1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_game_lists(eng, po, g64, n):
    from farkle_ii_amd.backend import COORD_DTYPE

    coords = np.zeros(n, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 10, 4711, 2, np.arange(n)
    seat = np.random.RandomState(100 + n).randint(0, 64, size=(n, 2)).astype(np.int32)
    want = po.play_games(coords.view(po.COORD_DTYPE), g64.view(po.STRATEGY_DTYPE), seat, 2).tobytes()
    for thr in THRESHOLDS:
        rows = _with_threshold(eng, thr, lambda: eng.play_games(coords, g64, seat, 2))
        assert eng.last_play_instance().endswith(", 2>")
        assert rows.tobytes() == want, thr


def test_safety_limit_games(eng, po, g64):
    """A pairing that never banks, max_rounds 3: every game ends at the round limit; nothing completes, no winner's record is tallied."""
    from farkle_ii_amd.backend import COL_COMPLETED, COL_SAFETY, COL_WINS

    never = _never_banking(g64)
    ref = po.tournament(never.view(po.STRATEGY_DTYPE), 2, 42, 0, 3, max_rounds=3, want_rows=True, n_threads=8)
    for thr in THRESHOLDS:
        counts = _with_threshold(eng, thr, lambda: eng.tournament(never, 2, 42, 0, 3, max_rounds=3))
        got = _with_threshold(eng, thr, lambda: eng.tournament(never, 2, 42, 0, 3, max_rounds=3, want_rows=True))
        assert np.array_equal(counts["tally"], ref["tally"]) and np.array_equal(got["tally"], ref["tally"]), thr
        assert got["rows"].tobytes() == ref["rows"].tobytes(), thr
        assert (counts["tally"][0][:, COL_SAFETY] == 3).all() and not counts["tally"][0][:, [COL_WINS, COL_COMPLETED]].any()


def test_a_call_without_rounds(eng, po, g64):
    """max_rounds 0: every dealt game has ended where it starts, so every hand-over is followed by a roll trip in which nobody plays."""
    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 3, max_rounds=0, want_rows=True, n_threads=8)
    for thr in THRESHOLDS:
        counts = _with_threshold(eng, thr, lambda: eng.tournament(g64, 2, 42, 0, 3, max_rounds=0))
        got = _with_threshold(eng, thr, lambda: eng.tournament(g64, 2, 42, 0, 3, max_rounds=0, want_rows=True))
        assert np.array_equal(counts["tally"], ref["tally"]) and np.array_equal(got["tally"], ref["tally"]), thr
        assert got["rows"].tobytes() == ref["rows"].tobytes(), thr


@pytest.mark.parametrize("form", ["uniform", "rb_fav", "all"])
def test_flag_forms(eng, po, g64, form):
    table = g64.copy()
    if form == "uniform":
        table["require_both"], table["favor_score"] = 1, 0
        table["score_threshold"], table["dice_threshold"] = 250 + 25 * (np.arange(64) // 4), np.arange(64) % 4
    elif form == "all":
        i = np.arange(64)
        table["smart_one"], table["auto_hot_dice"], table["run_up_score"] = (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), 2, 11, 0, 3, want_rows=True, n_threads=8)
    counts = eng.tournament(table, 2, 11, 0, 3)
    assert eng.timing()["play_mixed_flags"] == {"uniform": 0, "rb_fav": 0xc000, "all": 0xff00}[form] and eng.last_play_instance().endswith(", 2>")
    got = eng.tournament(table, 2, 11, 0, 3, want_rows=True)
    assert np.array_equal(counts["tally"], ref["tally"]) and np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()


def test_flat_and_general_hand_over_agree(eng, g64, ref5):
    """Option `flat_handover` 0 and 1: the two copies of the instance's loop nest, equal to each other and to the oracle in every output."""
    out = {}
    try:
        for flat in (0, 1):
            eng.set_option("flat_handover", flat)
            out[flat] = (eng.tournament(g64, 2, 42, 0, 5), eng.tournament(g64, 2, 42, 0, 5, shuffles_per_batch=1),
                         eng.tournament(g64, 2, 42, 0, 5, shuffles_per_batch=1, want_rows=True))
    finally:
        eng.set_option("flat_handover", 1)
    for flat in (0, 1):
        counts, batches, rows = out[flat]
        assert np.array_equal(counts["tally"][0], ref5["tally"].sum(axis=0)), flat
        assert np.array_equal(batches["tally"], ref5["tally"]), flat
        assert np.array_equal(rows["tally"], ref5["tally"]) and rows["rows"].tobytes() == ref5["rows"].tobytes(), flat
    assert np.array_equal(out[0][0]["tally"], out[1][0]["tally"]) and out[0][2]["rows"].tobytes() == out[1][2]["rows"].tobytes()
