"""The hand-over of the two-seat game kernel (round 10) — where a lane ends its game and starts the next one — bit-compared with the
CPU oracle at the smallest shapes at which it can go wrong.  fk_kernels.h: the flat path of the two-seat tournament / game-list instance
(`init_game2`, `finish_game2`, fk_device.h's `finish2_50`) and the general copy of its loop nest (option `flat_handover` 0); the hand-over
rule itself is the one of earlier rounds (threshold, nobody active, or tickets run out).  Covered: the ticket pool's edges, hand-overs
driven by every threshold with several games per lane, both schedules, every output kind (LDS tally, state store + result records,
`rec0` of a multi-batch call), games that do not complete (round limit, overrides, `max_rounds` 0), game lists around the wave size, the
H2H block instance (general path), the three strategy-flag forms and the forced-detour build.  A mistake in this code shows as a hang:
run this file alone, under a time limit of its own, before anything else that uses the changed kernel."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TWO_SEAT = "fk_play_kernel<768, true, 6, 49152u, false, false, 2>"  # the benchmark's instance (require_both | favor_score mixed)


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
def ref5(po, g64):
    """160 two-seat games (five shuffles), rows and per-shuffle tallies: computed once; the smaller pool-edge cases are its prefixes."""
    return po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 5, shuffles_per_batch=1, want_rows=True, n_threads=8)


@pytest.fixture(scope="module")
def ref40(po, g64):
    return po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 40, shuffles_per_batch=8, want_rows=True, n_threads=8)


def _never_banking(g64):
    never = g64.copy()
    never["dice_threshold"], never["require_both"] = 0, 1  # score AND dice below threshold never holds with 0 dice: no seat ever banks
    return never


@pytest.mark.parametrize("n_sh", [1, 2, 3, 5])
def test_ticket_pool_edges(eng, g64, ref5, n_sh):
    """32, 64, 96 and 160 games against chunks of 64 tickets: a partial first chunk, exactly one chunk, one and a half, and — in every
    case — waves that get no ticket at all (the grid has thousands) and must leave through the hand-over that deals nothing."""
    counts = eng.tournament(g64, 2, 42, 0, n_sh)
    assert eng.last_play_instance() == TWO_SEAT
    assert np.array_equal(counts["tally"][0], ref5["tally"][:n_sh].sum(axis=0))
    got = eng.tournament(g64, 2, 42, 0, n_sh, shuffles_per_batch=1, want_rows=True)
    assert np.array_equal(got["tally"], ref5["tally"][:n_sh])
    assert got["rows"].tobytes() == ref5["rows"][:32 * n_sh].tobytes()


@pytest.fixture(scope="module")
def long_call(eng, po, g64):
    """A call in which every lane of the smallest grid the two-seat instance runs on (one 768-thread block per CU) plays at least three
    games, so that most hand-overs are the threshold's: 3 x lanes / 32 shuffles (18 432 on 256 CUs; 6 000 shuffles would give that
    grid's 196 608 lanes less than one game each).  The oracle's tally is computed once."""
    n_sh = -(-3 * eng.device_info()["compute_units"] * 768 // 32)
    return n_sh, po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 7, 0, n_sh, n_threads=16)["tally"][0]


def test_threshold_driven_handovers(eng, g64, long_call):
    n_sh, want = long_call
    results = {}
    try:
        eng.set_option("block", 768)  # (with one block per CU the plan would otherwise prefer 1 024 lanes of full records)
        eng.set_option("blocks_per_cu", 1)
        for thr in (1, 2, 8, 64):
            eng.set_option("batch_threshold", thr)
            results[thr] = eng.tournament(g64, 2, 7, 0, n_sh)["tally"][0]
            t = eng.timing()
            assert eng.last_play_instance() == TWO_SEAT and t["play_block"] == 768
            assert 32 * n_sh >= 3 * t["play_grid"] * t["play_block"], (t["play_grid"], t["play_block"])  # three games per lane or more
    finally:
        eng.set_option("batch_threshold", 0)
        eng.set_option("blocks_per_cu", 0)
        eng.set_option("block", 0)
    for thr, tally in results.items():
        assert np.array_equal(tally, want), thr
        assert np.array_equal(tally, results[1]), thr


def test_without_a_schedule(eng, g64, long_call, ref40):
    """longest_first 0: no schedule, the state records at the slot computed from the game id (shuffle-minor walk order)."""
    n_sh, want = long_call
    try:
        eng.set_option("longest_first", 0)
        eng.set_option("block", 768)
        eng.set_option("blocks_per_cu", 1)
        long_tally = eng.tournament(g64, 2, 7, 0, n_sh)["tally"][0]
        assert eng.last_play_instance() == TWO_SEAT
        eng.set_option("blocks_per_cu", 0)
        eng.set_option("block", 0)
        got = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, want_rows=True)
        counts = eng.tournament(g64, 2, 42, 0, 40)
    finally:
        eng.set_option("longest_first", 1)
        eng.set_option("blocks_per_cu", 0)
        eng.set_option("block", 0)
    assert np.array_equal(long_tally, want)
    assert np.array_equal(got["tally"], ref40["tally"]) and got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(counts["tally"][0], ref40["tally"].sum(axis=0))


def test_every_output_kind(eng, g64, ref40):
    from oracle_engine_stub import seat_stats_from_rows

    counts = eng.tournament(g64, 2, 42, 0, 40)  # one batch, counts only: the LDS tally
    assert eng.last_play_instance() == TWO_SEAT and eng.timing()["play_lds_bytes"] > 2 * 768 * 40
    assert np.array_equal(counts["tally"][0], ref40["tally"].sum(axis=0))
    got = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, want_rows=True, want_seat_stats=True)  # state store + result records
    assert eng.last_play_instance() == TWO_SEAT
    assert np.array_equal(got["tally"], ref40["tally"]) and got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref40["rows"], 2, 64, 32, 8))
    assert int(got["seat_stats"][:, :, 0].sum()) == 40 * 64  # one exposure per seat per shuffle
    batches = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8)  # several batches, counts only: rec0 instead of the LDS tally
    assert eng.last_play_instance() == TWO_SEAT and eng.timing()["play_lds_bytes"] == 2 * 768 * 40
    assert np.array_equal(batches["tally"], ref40["tally"])


def test_games_that_end_at_the_round_limit(eng, po, g64):
    """Nobody banks: every game ends at max_rounds, every exposure is a safety-limit exposure, nothing completes."""
    from farkle_ii_amd.backend import COL_COMPLETED, COL_SAFETY, COL_WINS

    never = _never_banking(g64)
    for max_rounds in (1, 3):
        ref = po.tournament(never.view(po.STRATEGY_DTYPE), 2, 42, 0, 6, max_rounds=max_rounds, want_rows=True, n_threads=8)
        counts = eng.tournament(never, 2, 42, 0, 6, max_rounds=max_rounds)
        got = eng.tournament(never, 2, 42, 0, 6, max_rounds=max_rounds, want_rows=True)
        assert np.array_equal(counts["tally"], ref["tally"]) and np.array_equal(got["tally"], ref["tally"]), max_rounds
        assert got["rows"].tobytes() == ref["rows"].tobytes(), max_rounds
        assert (counts["tally"][0][:, COL_SAFETY] == 6).all() and not counts["tally"][0][:, [COL_WINS, COL_COMPLETED]].any()


def test_overrides_at_the_first_a_middle_and_the_last_game(eng, po, g64):
    """max_rounds overrides — 0 (no round is played), 1 and 2 — on game 0 of the first shuffle, a game in the middle and the last game of
    the last shuffle: found by the hand-over's binary search, in the LDS-tally launch, the multi-batch launch and with rows."""
    from farkle_ii_amd.backend import make_overrides

    ovs = [(42, 0, 0, 2, 0), (42, 19, 17, 2, 1), (42, 39, 31, 2, 2)]
    ref = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 40, shuffles_per_batch=8, overrides=po.make_overrides(ovs), want_rows=True,
                        n_threads=8)
    assert ref["tally"][:, :, 3].sum() >= 2  # the override to 0 rounds at least is a safety-limit game
    counts = eng.tournament(g64, 2, 42, 0, 40, overrides=make_overrides(ovs))
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))
    batches = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, overrides=make_overrides(ovs))
    assert np.array_equal(batches["tally"], ref["tally"])
    got = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, overrides=make_overrides(ovs), want_rows=True)
    assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes()
    zero = eng.tournament(g64, 2, 42, 0, 3, max_rounds=0)  # every game without a round
    assert np.array_equal(zero["tally"], po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 3, max_rounds=0, n_threads=8)["tally"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_game_lists(eng, po, g64, n):
    from farkle_ii_amd.backend import COORD_DTYPE

    coords = np.zeros(n, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 10, 321, 2, np.arange(n)
    rs = np.random.RandomState(n)
    seat = rs.randint(0, 64, size=(n, 2)).astype(np.int32)
    rows = eng.play_games(coords, g64, seat, 2)
    assert eng.last_play_instance().endswith(", 2>")
    assert rows.tobytes() == po.play_games(coords.view(po.COORD_DTYPE), g64.view(po.STRATEGY_DTYPE), seat, 2).tobytes()


def test_h2h_block_instance(eng, po, g64):
    """Three small blocks in one launch, one of them between two seats that never bank (its attempts all end at the round limit)."""
    never = _never_banking(g64)
    pairs = np.stack([g64[[3, 40]], never[[0, 2]], g64[[17, 9]]])
    got = eng.h2h_blocks(pairs, 42, [5, 6, 7], [0, 1, 0], 150, 300, max_rounds=20)
    assert eng.last_play_instance().endswith("true, 2>")  # BLK, two seats
    for b in range(3):
        want = po.h2h_block(pairs[b].view(po.STRATEGY_DTYPE), 42, 5 + b, [0, 1, 0][b], 150, 300, 300, max_rounds=20)
        assert np.array_equal(got[b], want), b


@pytest.mark.parametrize("form", ["uniform", "rb_fav", "all"])
def test_flag_forms(eng, po, g64, form):
    """The three instances by strategy flags: every flag shared by the table, require_both | favor_score mixed, every flag mixed."""
    table = g64.copy()
    if form == "uniform":
        table["require_both"], table["favor_score"] = 1, 0
        table["score_threshold"], table["dice_threshold"] = 250 + 25 * (np.arange(64) // 4), np.arange(64) % 4
    elif form == "all":
        i = np.arange(64)
        table["smart_one"], table["auto_hot_dice"], table["run_up_score"] = (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), 2, 9, 0, 12, want_rows=True, n_threads=8)
    counts = eng.tournament(table, 2, 9, 0, 12)
    want_mixed = {"uniform": 0, "rb_fav": 0xc000, "all": 0xff00}[form]
    assert eng.timing()["play_mixed_flags"] == want_mixed and eng.last_play_instance().endswith(", 2>")
    got = eng.tournament(table, 2, 9, 0, 12, want_rows=True)
    assert np.array_equal(counts["tally"], ref["tally"]) and np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()


def test_general_copy_of_the_loop_nest(eng, po, g64, ref40):
    """Option `flat_handover` 0: the launch enters the general copy of the two-seat instance's loop nest (what a chunk too large for
    32-bit record offsets takes) — same instance, same results, in every output kind and with overrides."""
    from farkle_ii_amd.backend import make_overrides

    ovs = [(42, 0, 0, 2, 0), (42, 19, 17, 2, 1), (42, 39, 31, 2, 2)]
    ref_ov = po.tournament(g64.view(po.STRATEGY_DTYPE), 2, 42, 0, 40, overrides=po.make_overrides(ovs), n_threads=8)
    try:
        eng.set_option("flat_handover", 0)
        counts = eng.tournament(g64, 2, 42, 0, 40)
        assert eng.last_play_instance() == TWO_SEAT
        got = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, want_rows=True)
        batches = eng.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8)
        with_ov = eng.tournament(g64, 2, 42, 0, 40, overrides=make_overrides(ovs))
    finally:
        eng.set_option("flat_handover", 1)
    assert np.array_equal(counts["tally"][0], ref40["tally"].sum(axis=0))
    assert np.array_equal(got["tally"], ref40["tally"]) and got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(batches["tally"], ref40["tally"])
    assert np.array_equal(with_ov["tally"], ref_ov["tally"])


def test_forced_detours(g64, ref40):
    """libfarkle_hip_detour.so (-DFK_FORCE_DETOUR=4): the same hand-over around a roll loop in which every fourth roll is replayed."""
    from farkle_ii_amd import backend

    backend.build_library(variant="detour")  # prebuilt by __graft_entry__.build()
    detour = backend.Engine(0, variant="detour")
    try:
        got = detour.tournament(g64, 2, 42, 0, 40, shuffles_per_batch=8, want_rows=True)
        counts = detour.tournament(g64, 2, 42, 0, 40)
    finally:
        detour.close()
    assert np.array_equal(got["tally"], ref40["tally"]) and got["rows"].tobytes() == ref40["rows"].tobytes()
    assert np.array_equal(counts["tally"][0], ref40["tally"].sum(axis=0))
