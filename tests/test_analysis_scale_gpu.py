"""The game-stats, rare-event and seat-analysis post-passes on the MI355X at the production table and at launch sizes where their
code paths change (``analysis_scale_cases.py``: permutation images in blocks of 15 shuffles, an event scan of several waves and of
two tiles, a second trip of the record kernels' grid-stride loop, seat counts over 21 workgroups, more than 65 536 mirrored pairs
with 13-bit ID ranks), and with ``longest_first`` off (the state-reading post-passes then take ``walk_slot``).  Every comparison is
exact, against the oracle-backed stubs plus the host statements."""
from __future__ import annotations

import numpy as np
import pytest

import analysis_scale_cases as asc
from oracle_engine_stub import column_images
from rare_events_engine_stub import Engine as RareStub
from seat_analysis_engine_stub import Engine as SeatStub
from test_game_stats_gpu import _same as _same_game_stats
from test_rare_events_gpu import _same
from test_seat_analysis_gpu import _ids, _same_counts, _same_pairs

from farkle_ii_amd import game_stats as gs
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError, make_overrides

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _ascending(res: dict, name: str) -> None:
    ids = asc.event_ids(res, name)
    assert len(ids) == res["rare_events"]["events"] and np.all(np.diff(ids) > 0)  # strictly ascending in (shuffle, game)


# ---------------------------------------------------------------------------------------------------------- rare events
@pytest.mark.parametrize("name", list(asc.RARE_CASES))
def test_hip_rare_events_equal_the_stub_at_scale(eng, name):
    fig = asc.check_rare_preconditions(name)
    got = asc.rare_call(eng, name, event_capacity=10 ** 6)
    print(name, fig, "attempts", got["attempts"], "spilled", got["spilled"])
    assert got["attempts"] == 1
    _same(got, asc.rare_want(name))
    _ascending(got, name)


def test_hip_dense_list_beyond_the_default_event_capacity(eng):
    """Two tiles of the scan with every block full, into a list that is 65 536 entries short at first."""
    fig = asc.check_rare_preconditions("two_tiles_dense")
    assert fig["events"] > 65_536
    got = asc.rare_call(eng, "two_tiles_dense", retry=True)  # event_capacity: the default
    assert got["attempts"] == 2
    _same(got, asc.rare_want("two_tiles_dense"))
    _ascending(got, "two_tiles_dense")


def test_hip_dense_list_over_many_small_chunks(eng):
    """The smallest workspace: four-shuffle chunks, the running event total carried across dozens of them to a base above 2^17."""
    fig = asc.check_rare_preconditions("two_tiles_dense")
    assert fig["events"] > 1 << 17
    eng.set_option("chunk_bytes", 1 << 20)
    try:
        chunked = asc.rare_call(eng, "two_tiles_dense", event_capacity=10 ** 6)
        launches = eng.timing()["play_launches"]
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    print("play_launches", launches)
    assert launches >= 20
    whole = asc.rare_call(eng, "two_tiles_dense", event_capacity=10 ** 6)
    assert eng.timing()["play_launches"] == 1
    _same(chunked, whole)
    _same(chunked, asc.rare_want("two_tiles_dense"))
    _ascending(chunked, "two_tiles_dense")


@pytest.mark.parametrize("name", ["grid_stride", "hot_cold_k12"])
def test_hip_game_stats_alone_equal_the_stub_at_scale(eng, name):
    asc.check_rare_preconditions(name)
    got = asc.game_stats_call(eng, name)
    assert got["spilled"] == 0
    _same_game_stats(got, asc.rare_want(name))  # (the seven outputs and the tally: the stub's rare-events result holds them)


# -------------------------------------------------------------------------------------------------------- seat analysis
@pytest.mark.parametrize("name", list(asc.SEAT_CASES))
def test_hip_seat_analysis_equals_the_stub_at_scale(eng, name):
    fig = asc.check_seat_preconditions(name)
    want = asc.seat_want(name)
    got = asc.seat_call(eng, name)
    print(name, fig, "attempts", got["attempts"])
    _same_counts(got, want)
    if not asc.SEAT_CASES[name]["mirrored"]:
        assert got["pair_index"] is None and got["pair_sums"] is None
        return
    _same_pairs(got, want)
    sums = got["pair_sums"]
    if name == "pairs_5160":
        assert got["attempts"] == 1 and len(sums) > 65_536
        assert (sums[:, 2] + sums[:, 3]).sum() == fig["games"]  # every game is in exactly one row
        n = len(sums)
        with pytest.raises(FarkleHipError) as err:
            asc.seat_call(eng, name, pair_capacity=n - 1, retry=False)
        assert err.value.code == FK_ERR_ARG and err.value.pairs_needed == n
    else:
        assert got["attempts"] == 1 and len(sums) <= 65_536  # (the default capacity holds every pair of 300 strategies)


# ---------------------------------------------------------------------------------------------------- longest_first = 0
def _small_table(S: int):
    from tools.time_config import table_for

    return table_for(S)


def _defined(columns: np.ndarray, k: int, gps: int) -> np.ndarray:
    return columns[:, :((4 + 13 * k) * 4 + 2 + k) * gps]  # (an image is padded to a multiple of 64 bytes; nothing reads the padding)


@pytest.mark.parametrize("S,k", [(120, 2), (120, 4), (120, 12), (64, 2), (64, 4)])
def test_hip_post_passes_without_the_inverted_schedule(eng, S, k):
    """``longest_first = 0``: the game kernel deals games in walk order and the post-passes that read the state store find a
    game's records by ``walk_slot`` — game-stats records, second scores, the all-player statistics and the column images."""
    t = _small_table(S)
    ov = make_overrides([(42, 3, 0, k, 2), (42, 7, 1, k, 1), (42, 11, 2, k, 3)])  # safety-limit games
    play = dict(shuffles_per_batch=16, overrides=ov, target_score=3000)
    kw = dict(play, rare_target_score=2000)
    ids = _ids(S)
    stub = RareStub()
    want = stub.tournament_rare_events(t, k, 42, 0, 40, thresholds=(500, 1000), want_seat_stats=True, **kw)
    want_columns = stub.tournament_columns(t, k, 42, 0, 40, ids, **play)
    want_seats = SeatStub().tournament_seat_counts(t, k, 42, 0, 40, strategy_ids=ids, want_mirrored=k == 2, **play)
    assert want["rare_events"]["events"] > 0 and want["game_stats"]["game_counts"][gs.SAFETY] >= 2

    def run():
        return (eng.tournament_rare_events(t, k, 42, 0, 40, thresholds=(500, 1000), want_seat_stats=True, **kw),
                eng.tournament_game_stats(t, k, 42, 0, 40, want_seat_stats=True, **kw),
                eng.tournament_seat_counts(t, k, 42, 0, 40, strategy_ids=ids, want_mirrored=k == 2, **play),
                eng.tournament_columns(t, k, 42, 0, 40, ids, **play))

    before = run()
    eng.set_option("longest_first", 0)
    try:
        off = run()
    finally:
        eng.set_option("longest_first", 1)
    after = run()
    for rare, stats, seats, columns in (off, before, after):
        _same(rare, want)
        _same_game_stats(stats, want)
        for res in (rare, stats):
            assert np.array_equal(res["seat_stats"], want["seat_stats"])
            assert res["seat_ratio_sums"].tobytes() == want["seat_ratio_sums"].tobytes()
        _same_counts(seats, want_seats)
        if k == 2:
            _same_pairs(seats, want_seats)
        assert np.array_equal(columns["tally"], want_columns["tally"])
        assert np.array_equal(_defined(columns["columns"], k, S // k), _defined(want_columns["columns"], k, S // k))
    # a plain call with the option restored equals its earlier self, byte for byte
    for a, b in zip(before, after):
        assert np.array_equal(a["tally"], b["tally"])
    assert np.array_equal(before[0]["rare_events"]["event_head"], after[0]["rare_events"]["event_head"])
    assert np.array_equal(before[0]["rare_events"]["event_seats"], after[0]["rare_events"]["event_seats"])
    assert np.array_equal(_defined(before[3]["columns"], k, S // k), _defined(after[3]["columns"], k, S // k))
