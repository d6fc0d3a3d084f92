"""The roll loop of the two-seat lean game kernels since round 14: the Lemire replay, the `raise` block and the sampled guards sit out of
line behind a wave-uniform test of the mask they run under, and a trip in which no lane's game ended and no lane raised goes round on
one compare of the playing lanes' mask with its value at the last full hand-over test; popcount, threshold and `exhausted` run only
on a trip that changed the masks, and once after a hand-over that left ended lanes behind.  Every case compares with the CPU oracle
for the same call (tallies; rows where the case reads them), on the product library and on the forced-detour build, where the
out-of-line replay runs every fourth roll.  Covered: game counts that leave never-dealt lanes, a partial last ticket chunk and a wave
that drains while others play; batch thresholds 1, 8 and 64 on both copies of the loop nest; hand-overs after which nobody plays
(every dealt game has max_rounds 0), alone and mixed with default games in one wave; a two-strategy table with a low target, where
several lanes end in one trip; calls of fewer and of more than 32 trips per wave (the sampled guard runs zero times and many times);
a lane that raises from the sampled guard while its neighbours play on, and the next call on the same context; the batched H2H entry.

The raising lane: FK_ERR_ROLL_LIMIT needs a turn of 1 000 rolls, and no strategy pair is known that plays one (a never-banking seat
rolls until it farkles: tests/test_roll_bookkeeping_gpu.py, tests/test_trace_gpu.py); what tests/counter_limit_cases.py builds from a
never-banking pairing is a seat one roll beyond the 64 000-rolls band, which these instances find at a sample point of the roll loop
— the moved block — and report as FK_ERR_COUNTER_OVERFLOW.  That is the code asserted here.
A mistake in this code can show as a hang: run this file under a time limit of its own."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import counter_limit_cases as clc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "detour"])
def eng(request):
    from farkle_ii_amd import backend

    if request.param == "detour":
        backend.build_library(variant="detour")  # prebuilt by __graft_entry__.build()
    e = backend.Engine(0, variant=None if request.param == "product" else "detour")
    yield e
    e.set_option("batch_threshold", 0)
    e.set_option("flat_handover", 1)
    e.close()


@lru_cache(maxsize=None)
def _g64() -> np.ndarray:
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies

    strategies, _ = generate_strategy_grid(
        score_thresholds=[250, 300, 350, 400], dice_thresholds=[0, 1, 2, 3], smart_five_opts=[True], smart_one_opts=[True],
        consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[True])
    table = pack_strategies(strategies)
    assert len(table) == 64
    return table


@lru_cache(maxsize=None)
def _table(name: str) -> np.ndarray:
    if name == "g64":
        return _g64()
    t = _g64()[[5, 46]].copy()  # "pair": two strategies, one game per shuffle; the seats differ in require_both
    t["favor_score"] = 1
    t["require_both"] = (1, 0)
    return t


@lru_cache(maxsize=None)
def _ref(name: str, seed: int, n_sh: int, items: tuple = (), **kw):
    """The oracle's result, computed once per call and shared by both libraries' cases (nobody writes into it)."""
    import pyoracle as po

    if items:
        kw["overrides"] = po.make_overrides(list(items))
    return po.tournament(_table(name).view(po.STRATEGY_DTYPE), 2, seed, 0, n_sh, want_rows=True, n_threads=8, **kw)


def _same(eng, name: str, seed: int, n_sh: int, items: tuple = (), rows: bool = True, **kw) -> dict:
    from farkle_ii_amd.backend import make_overrides

    ref = _ref(name, seed, n_sh, items, **kw)
    call = dict(kw, overrides=make_overrides(list(items))) if items else kw
    counts = eng.tournament(_table(name), 2, seed, 0, n_sh, **{a: v for a, v in call.items() if a != "shuffles_per_batch"})
    assert eng.last_play_instance().endswith(", 2>"), eng.last_play_instance()
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))
    if rows:
        got = eng.tournament(_table(name), 2, seed, 0, n_sh, want_rows=True, **call)
        assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 769, 1537])
def test_game_counts(eng, n):
    """One game per shuffle: waves with never-dealt lanes (1, 63, 65), a partial last ticket chunk, and with 769 and 1 537 games a wave that
    is dealt one game and drains while the block's other waves play."""
    _same(eng, "pair", 77, n, shuffles_per_batch=max(n // 3, 1))


@pytest.mark.parametrize("thr", [1, 8, 64])
@pytest.mark.parametrize("flat", [1, 0])
def test_batch_thresholds_on_both_copies_of_the_loop_nest(eng, thr, flat):
    """800 games.  Threshold 1: the hand-over is due on the first ended lane; 64: only when the last playing lane ends."""
    try:
        eng.set_option("batch_threshold", thr)
        eng.set_option("flat_handover", flat)
        _same(eng, "g64", 42, 25, shuffles_per_batch=5)
    finally:
        eng.set_option("batch_threshold", 0)
        eng.set_option("flat_handover", 1)


@pytest.mark.parametrize("flat", [1, 0])
def test_a_hand_over_after_which_nobody_plays(eng, flat):
    """max_rounds 0 for the whole call: every dealt game has ended where it is dealt, so each hand-over is followed by a trip without a
    playing lane and by the next hand-over, until the tickets run out."""
    try:
        eng.set_option("flat_handover", flat)
        ref = _same(eng, "g64", 42, 30, max_rounds=0, shuffles_per_batch=10)  # 960 games: more than one ticket chunk per wave
        assert (ref["rows"]["n_rounds"] == 0).all()
    finally:
        eng.set_option("flat_handover", 1)


@pytest.mark.parametrize("thr,flat", [(0, 1), (1, 1), (64, 1), (0, 0)])
def test_games_without_rounds_beside_default_games_in_one_wave(eng, thr, flat):
    """Overrides give every third game of 96 max_rounds 0 and every seventh max_rounds 1: a hand-over leaves ended lanes behind while
    others play, so the first trip after it is followed by the full test whatever that trip changed."""
    items = tuple((42, sh, g, 2, 0 if (32 * sh + g) % 3 == 0 else 1) for sh in range(3) for g in range(32) if (32 * sh + g) % 3 == 0 or (32 * sh + g) % 7 == 0)
    try:
        eng.set_option("batch_threshold", thr)
        eng.set_option("flat_handover", flat)
        ref = _same(eng, "g64", 42, 3, items)
        assert (ref["rows"]["n_rounds"] == 0).sum() == 32 and (ref["rows"]["n_rounds"] > 1).any()
    finally:
        eng.set_option("batch_threshold", 0)
        eng.set_option("flat_handover", 1)


@pytest.mark.parametrize("thr", [0, 1, 64])
def test_short_table_with_a_low_target(eng, thr):
    """Two strategies, target 500: the first banked turn starts the final round, games end within the wave's first trips and several
    lanes end in the same trip (threshold 0 is the automatic value, 8: they cross it together)."""
    try:
        eng.set_option("batch_threshold", thr)
        ref = _same(eng, "pair", 9, 200, target_score=500, shuffles_per_batch=50)
        assert np.median(ref["rows"]["n_rounds"]) <= 3
    finally:
        eng.set_option("batch_threshold", 0)


def test_a_call_shorter_than_one_sample_interval(eng):
    """64 games of one round, all dealt to one wave in its first hand-over: a lane plays as many trips as its game has rolls, and the
    oracle's rows show that no game has 32, so the wave ends before its first sample point and the sampled guard never runs."""
    ref = _same(eng, "pair", 5, 64, max_rounds=1, target_score=500)
    assert len(ref["rows"]) == 64 and ref["rows"]["seats"]["rolls"].astype(np.int64).sum(axis=1).max() < 32


def test_a_call_of_many_sample_intervals(eng):
    """Default games (some fifty rolls each, several per lane): the sampled guard runs many times and finds nothing."""
    _same(eng, "g64", 11, 40, shuffles_per_batch=8)


LONG_GAMES = range(16, 36)  # games 16 ... 35 of shuffle 1 of the call: tickets 64 ... 83, inside one 64-ticket chunk, so one wave is dealt them all


def _total_rolls(row) -> int:
    """Both seats' rolls: the trips the game's lane plays, since every playing lane rolls once a trip."""
    return int(row["seats"]["rolls"].astype(np.int64).sum())


@lru_cache(maxsize=None)
def _raising_case() -> dict:
    """tests/counter_limit_cases.py's never-banking table and call, with twenty long games side by side: each has its own last round
    limit inside the 64 000-rolls band (``R_in``; one round more, ``R_out``, and a seat is beyond it).  The offender is the one of them
    that leaves the band EARLIEST in trips — its seats are the most unequal — and ``outlast`` are the others whose lanes still play when
    it raises: a lane has played as many trips as its game has rolls (all of them are dealt in their wave's first hand-over), the
    offender's seat passes the band within round ``R_out``, and the sample point that hears it comes at most 32 trips later."""
    import pyoracle as po

    table, C = clc.never_bank_table("none", 96), clc.CALL
    sh = clc.OFFENDER_SHUFFLE
    long_games = {g: clc.boundary(table, 2, clc.ROOT, sh, g, "rolls", clc.PLAY_ROLLS_LIMIT, guess=16_000) for g in LONG_GAMES}
    assert all(b["row_out"] is not None for b in long_games.values())
    off = min(long_games, key=lambda g: _total_rolls(long_games[g]["row_out"]))
    raised_by = _total_rolls(long_games[off]["row_out"]) + 32
    outlast = [g for g, b in long_games.items() if g != off and _total_rolls(b["row_in"]) > raised_by]
    neighbours = [clc.game_override(clc.ROOT, sh, g, 2, b["R_in"]) for g, b in long_games.items() if g != off]
    ref = po.tournament(np.ascontiguousarray(table).view(po.STRATEGY_DTYPE), 2, clc.ROOT, C["begin"], C["end"], shuffles_per_batch=C["spb"],
                        max_rounds=C["max_rounds"], overrides=po.make_overrides(neighbours + [clc.game_override(clc.ROOT, sh, off, 2, long_games[off]["R_in"])]),
                        want_rows=True, n_threads=8)
    return {"table": table, "offender": (sh, off), "game": (sh - C["begin"]) * (96 // 2) + off, "R_in": long_games[off]["R_in"], "R_out": long_games[off]["R_out"],
            "neighbours": neighbours, "outlast": outlast, "ref": ref}


@pytest.mark.parametrize("flat", [1, 0])
def test_a_lane_raises_from_the_sampled_guard_while_its_neighbours_play_on(eng, flat):
    """One game is played to the last round inside the 64 000-rolls band (the call equals the oracle), then one round further: the error,
    naming that game, raised at a sample point of the roll loop.  Nineteen games on the tickets around it are as long (each to its own last
    round inside the band), and several of them have more rolls than the offender has when it raises: their lanes are in m_active then,
    so the raise takes one lane out of a mask that stays non-zero, the trip goes into the full hand-over test, and the loop goes on.
    Then the first call again on the same context."""
    from farkle_ii_amd.backend import FK_ERR_COUNTER_OVERFLOW, FarkleHipError, make_overrides

    case, C = _raising_case(), clc.CALL
    ref = case["ref"]
    assert len(case["outlast"]) >= 3, case["outlast"]  # (on the oracle's rows: lanes that play on when the offender raises)

    def call(rounds, **kw):
        ov = make_overrides(case["neighbours"] + [clc.game_override(clc.ROOT, *case["offender"], 2, rounds)])
        return eng.tournament(case["table"], 2, clc.ROOT, C["begin"], C["end"], shuffles_per_batch=C["spb"], max_rounds=C["max_rounds"], overrides=ov, **kw)

    try:
        eng.set_option("flat_handover", flat)
        for attempt in ("first", "after the error"):
            got = call(case["R_in"], want_rows=True)
            assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes(), attempt
            assert np.array_equal(call(case["R_in"])["tally"], ref["tally"]), attempt  # (counts only: one tally per batch, as the oracle's)
            if attempt == "first":
                for wanted in (dict(want_rows=True), {}):
                    with pytest.raises(FarkleHipError) as err:
                        call(case["R_out"], **wanted)
                    assert err.value.code == FK_ERR_COUNTER_OVERFLOW, str(err.value)
                    assert f"game {case['game']})" in str(err.value), str(err.value)
    finally:
        eng.set_option("flat_handover", 1)


def test_batched_head_to_head_with_a_pairing_at_the_round_limit(eng):
    """The block instance.  Two blocks of 2 000 attempts: a pairing that completes its games, and two never-banking seats whose games all run to the limit."""
    never = _g64()[[3, 40]].copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    pairs = np.stack([_g64()[[3, 40]], never])
    got = eng.h2h_blocks(pairs, 42, [5, 6], [0, 1], 2000, 2000, target_score=2000, max_rounds=12)
    for b in range(2):
        assert np.array_equal(got[b], _h2h_reference(b)), b
    assert got[1][2] == 2000 and got[1][1] == 0 and got[0][1] > 0  # (attempted, completed, safety, wins 1, wins 2)


@lru_cache(maxsize=None)
def _h2h_reference(b: int):
    import pyoracle as po

    never = _g64()[[3, 40]].copy()
    never["dice_threshold"], never["require_both"] = 0, 1
    pairs = np.stack([_g64()[[3, 40]], never])
    return po.h2h_block(pairs[b].view(po.STRATEGY_DTYPE), 42, 5 + b, b, 2000, 2000, 2000, target_score=2000, max_rounds=12)
