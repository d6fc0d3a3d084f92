"""The two-seat lean game kernels carry the per-lane game flags (playing, ended, final round, the owner's seat) as wave-uniform lane
masks since round 13, and a roll trip is run by every lane of the wave: the masks decide which lanes store their roll and advance.
Every case here compares the tally with the CPU oracle for the same call; one case per strategy-flag form also compares the rows and
the all-seat statistics, which are read from the final state records of every seat (scores, n_turns, has_scored's effects).  Covered:
game counts that leave partial waves and partial ticket chunks; max_rounds 0 (every game ended where it is dealt), 1 and 2; round
overrides that mix 0 and the default inside one wave; a low target, where the first banked turn triggers the final round, from either
seat; two-strategy tables whose seats differ, or agree, in require_both, in the three flag forms; batch thresholds 1 and 64; the
general copy of the loop nest (`flat_handover` 0); one batched head-to-head call, one of its pairings running to the round limit.
A mistake in this code can show as a hang: run this file under a time limit of its own."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _pair(g64, form: str, rb: tuple[int, int]) -> np.ndarray:
    """A two-strategy table in one of the three flag forms whose seats hold require_both = rb."""
    t = g64[[5, 46]].copy()
    t["favor_score"] = 1
    t["require_both"] = rb
    if form == "uniform":  # no flag differs inside the table
        assert rb[0] == rb[1]
    elif form == "all":  # a flag outside require_both | favor_score differs too
        t["smart_one"] = (1, 0)
    elif rb[0] == rb[1]:  # "rb_fav" with equal require_both: favor_score is the bit that differs
        t["favor_score"] = (1, 0)
    return t


MIXED = {"uniform": (0,), "rb_fav": (0x4000, 0x8000, 0xc000), "all": (0xff00,)}


def _both(eng, po, table, k, seed, n_sh, **kw):
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, seed, 0, n_sh, n_threads=8, **{a: v for a, v in kw.items() if a != "want_seat_stats"})
    got = eng.tournament(table, k, seed, 0, n_sh, **kw)
    assert eng.last_play_instance().endswith(", 2>"), eng.last_play_instance()
    return got, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 769])
def test_game_counts_around_the_wave_and_the_ticket_chunk(eng, po, g64, n):
    """S = 2: one game per shuffle, so n shuffles are n games; the table's seats differ in require_both (rb_delta set in every game)."""
    table = _pair(g64, "rb_fav", (1, 0))
    got, ref = _both(eng, po, table, 2, 77, n)
    assert np.array_equal(got["tally"], ref["tally"])
    got, ref = _both(eng, po, table, 2, 77, n, shuffles_per_batch=max(n // 3, 1), want_rows=True)
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()


@pytest.mark.parametrize("max_rounds", [0, 1, 2])
def test_round_limits(eng, po, g64, max_rounds):
    got, ref = _both(eng, po, g64, 2, 42, 3, max_rounds=max_rounds)
    assert np.array_equal(got["tally"], ref["tally"])
    got, ref = _both(eng, po, g64, 2, 42, 3, max_rounds=max_rounds, want_rows=True)
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()


def test_overrides_mix_no_rounds_and_the_default_in_one_wave(eng, po, g64):
    """Every third game of 96 (two waves' worth of lanes in one block) is given max_rounds 0, every seventh max_rounds 1."""
    from farkle_ii_amd.backend import make_overrides

    items = [(42, sh, g, 2, 0 if (32 * sh + g) % 3 == 0 else 1) for sh in range(3) for g in range(32) if (32 * sh + g) % 3 == 0 or (32 * sh + g) % 7 == 0]
    ov = make_overrides(items)  # (root_seed, shuffle, game, k, max_rounds)
    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 3, overrides=po.make_overrides(items), want_rows=True, n_threads=8)
    got = eng.tournament(g64, 2, 42, 0, 3, overrides=ov, want_rows=True)
    counts = eng.tournament(g64, 2, 42, 0, 3, overrides=ov)
    assert np.array_equal(counts["tally"], ref["tally"])
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()
    assert (ref["rows"]["n_rounds"] == 0).sum() == 32 and (ref["rows"]["n_rounds"] > 1).any()


def test_low_target_triggers_from_either_seat(eng, po, g64):
    """Target 500: the first banked turn reaches it.  The seat that triggers plays no final turn, so in a completed game seat 0 has
    n_rounds turns when it triggered and n_rounds + 1 when seat 1 did."""
    from oracle_engine_stub import seat_stats_from_rows

    got, ref = _both(eng, po, g64, 2, 9, 4, target_score=500, shuffles_per_batch=2, want_rows=True, want_seat_stats=True)
    rows = ref["rows"]
    done = rows["status"] == 0
    t0, rounds = rows["seats"][:, 0]["n_turns"].astype(np.int64), rows["n_rounds"].astype(np.int64)
    assert (done & (t0 == rounds)).any(), "no game in which seat 0 triggers the final round"
    assert (done & (t0 == rounds + 1)).any(), "no game in which seat 1 triggers the final round"
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == rows.tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(rows, 2, 64, 32, 2))
    counts = eng.tournament(g64, 2, 9, 0, 4, target_score=500)
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))


@pytest.mark.parametrize("form,rb", [("uniform", (1, 1)), ("uniform", (0, 0)), ("rb_fav", (1, 0)), ("rb_fav", (0, 1)), ("rb_fav", (1, 1)),
                                     ("all", (1, 0)), ("all", (0, 0))])
def test_require_both_differs_or_agrees_in_every_flag_form(eng, po, g64, form, rb):
    """200 games of a two-strategy table: tally, rows and the all-seat statistics (from the final state records of both seats)."""
    from oracle_engine_stub import seat_stats_from_rows

    table = _pair(g64, form, rb)
    got, ref = _both(eng, po, table, 2, 31, 200, shuffles_per_batch=50, want_rows=True, want_seat_stats=True)
    assert eng.timing()["play_mixed_flags"] in MIXED[form], hex(eng.timing()["play_mixed_flags"])
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref["rows"], 2, 2, 1, 50))
    counts = eng.tournament(table, 2, 31, 0, 200)
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))


@pytest.mark.parametrize("thr", [1, 64])
@pytest.mark.parametrize("flat", [1, 0])
def test_batch_thresholds_and_both_copies_of_the_loop_nest(eng, po, g64, thr, flat):
    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 25, shuffles_per_batch=5, want_rows=True, n_threads=8)  # 800 games
    try:
        eng.set_option("batch_threshold", thr)
        eng.set_option("flat_handover", flat)
        counts = eng.tournament(g64, 2, 42, 0, 25)
        got = eng.tournament(g64, 2, 42, 0, 25, shuffles_per_batch=5, want_rows=True)
    finally:
        eng.set_option("batch_threshold", 0)
        eng.set_option("flat_handover", 1)
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()


def test_batched_head_to_head_with_a_pairing_at_the_round_limit(eng, po, g64):
    """Two blocks of 2 000 attempts: a pairing that completes its games, and two never-banking seats whose games all run to the limit."""
    never = g64[[3, 40]].copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    pairs = np.stack([g64[[3, 40]], never])
    got = eng.h2h_blocks(pairs, 42, [5, 6], [0, 1], 2000, 2000, target_score=2000, max_rounds=12)
    for b in range(2):
        want = po.h2h_block(pairs[b].view(po.STRATEGY_DTYPE), 42, 5 + b, b, 2000, 2000, 2000, target_score=2000, max_rounds=12)
        assert np.array_equal(got[b], want), b
    assert got[1][2] == 2000 and got[1][1] == 0 and got[0][1] > 0  # (attempted, completed, safety, wins 1, wins 2)
