"""The rare-event game list and second-score histograms on the MI355X: ``fk_tournament_run_rare_events`` against the host statement
over the oracle's rows, exact equality everywhere — every seat count up to twelve, a sparse, a mixed, a dense and an empty list,
workspace chunks and split calls (order is part of the contract), forced second-score spills, the capacity convention, the
game-stats outputs of the same launch, and every fixture case end to end."""
from __future__ import annotations

import numpy as np
import pytest

from rare_events_engine_stub import Engine as StubEngine
from test_rare_events_cpu import CASES, check_case

from farkle_ii_amd import game_stats as gs
from farkle_ii_amd import rare_events as rev
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError, make_overrides

pytestmark = pytest.mark.gpu

NAMES = ("strategy_counts", "strategy_rounds", "strategy_runner", "strategy_spread", "game_counts", "game_rounds", "game_runner")
SPARSE = dict(k=4, root_seed=9, shuffle_begin=100, shuffle_end=700, max_rounds=12, thresholds=(500, 1000))


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _table(S: int):
    from tools.time_config import table_for

    return table_for(S)


def _eq(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    n = max(a.shape[-1], b.shape[-1])
    pad = lambda x: gs._add_padded(x, np.zeros(x.shape[:-1] + (n,), np.int64))  # noqa: E731
    return np.array_equal(pad(a), pad(b))


def _same(got: dict, want: dict) -> None:
    """Event arrays, both second-score histograms, the seven game-stat outputs and the tally."""
    g, w = got["rare_events"], want["rare_events"]
    assert g["events"] == w["events"] == len(g["event_head"])
    assert np.array_equal(g["event_head"], w["event_head"])
    assert np.array_equal(g["event_seats"], w["event_seats"])
    assert _eq(g["strategy_second"], w["strategy_second"]) and _eq(g["game_second"], w["game_second"])
    for name in NAMES:
        assert _eq(got["game_stats"][name], want["game_stats"][name]), name
    assert np.array_equal(got["tally"], want["tally"])


@pytest.fixture(scope="module")
def sparse_want():
    kw = dict(SPARSE)
    return StubEngine().tournament_rare_events(_table(64), kw.pop("k"), kw.pop("root_seed"), kw.pop("shuffle_begin"), kw.pop("shuffle_end"), **kw)


def _sparse(eng, a=100, b=700, **extra):
    kw = dict(SPARSE, shuffle_begin=a, shuffle_end=b, **extra)
    return eng.tournament_rare_events(_table(64), kw.pop("k"), kw.pop("root_seed"), kw.pop("shuffle_begin"), kw.pop("shuffle_end"), **kw)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_hip_equals_the_host_statement_over_oracle_rows(eng, k):
    t = _table(120)
    ov = make_overrides([(42, 3, 0, k, 2), (42, 7, 1, k, 1), (42, 11, 2, k, 3)])  # safety-limit games
    kw = dict(shuffles_per_batch=16, overrides=ov, rare_target_score=2000, target_score=3000)
    want = StubEngine().tournament_rare_events(t, k, 42, 0, 40, thresholds=(500, 1000), **kw)
    got = eng.tournament_rare_events(t, k, 42, 0, 40, thresholds=(500, 1000), want_seat_stats=True, **kw)
    _same(got, want)
    n_games = 40 * (120 // k)
    assert got["rare_events"]["events"] < n_games  # unflagged games at every k
    assert (got["rare_events"]["events"] == 0) == (k == 1)
    if k == 1:
        assert got["rare_events"]["game_second"].sum() == 0 and got["rare_events"]["strategy_second"].sum() == 0
    else:
        assert got["rare_events"]["game_second"].sum() == n_games  # safety-limit games count
        f = rev.event_fields(got["rare_events"]["event_head"])
        assert np.all(f["multi"] | (f["mask"] != 0)) and np.all(np.diff(f["shuffle"] * (120 // k) + f["game"]) > 0)
    assert rev.tail_equals_multi_target(rev.RareEventSummary.from_engine(got, k), 2000)
    # the seven existing outputs, the tally and the all-player arrays equal tournament_game_stats of the same range
    base = eng.tournament_game_stats(t, k, 42, 0, 40, want_seat_stats=True, **kw)
    for name in NAMES:
        assert np.array_equal(got["game_stats"][name], base["game_stats"][name]), name
    assert np.array_equal(got["tally"], base["tally"]) and np.array_equal(got["seat_stats"], base["seat_stats"])
    assert got["seat_ratio_sums"].tobytes() == base["seat_ratio_sums"].tobytes()


def test_hip_sparse_list(eng, sparse_want):
    n = sparse_want["rare_events"]["events"]
    assert 0 < n < 96  # fewer than 1 % of the 9 600 games: most waves hold no event
    _same(_sparse(eng), sparse_want)


def test_hip_mixed_list(eng):
    t = _table(64)
    want = StubEngine().tournament_rare_events(t, 2, 5, 0, 64, thresholds=(500, 1000))
    f = rev.event_fields(want["rare_events"]["event_head"])
    assert np.any(f["multi"] & (f["mask"] == 0)) and np.any(~f["multi"]) and 0 < len(f["multi"]) < 2048
    _same(eng.tournament_rare_events(t, 2, 5, 0, 64, thresholds=(500, 1000)), want)


def test_hip_dense_and_empty_lists(eng):
    t = _table(64)
    kw = dict(target_score=3000, max_rounds=9)  # some games end at the safety limit
    dense_thr = (-50, 2 ** 31 - 1)  # a threshold >= every margin flags every completed game; a negative one flags none
    want = StubEngine().tournament_rare_events(t, 4, 9, 0, 30, rare_target_score=10 ** 6, thresholds=dense_thr, **kw)
    got = eng.tournament_rare_events(t, 4, 9, 0, 30, rare_target_score=10 ** 6, thresholds=dense_thr, event_capacity=4, **kw)
    _same(got, want)
    completed = int(got["game_stats"]["game_counts"][gs.COMPLETED])
    assert got["attempts"] == 2 and got["rare_events"]["events"] == completed and 0 < completed < 30 * 16
    assert np.all(rev.event_fields(got["rare_events"]["event_head"])["mask"] == 2)
    # no thresholds and a rare target above every score: zero events, the histograms only
    for want_events in (True, False):
        empty = eng.tournament_rare_events(t, 4, 9, 0, 30, rare_target_score=10 ** 6, thresholds=(), want_events=want_events, **kw)
        assert empty["rare_events"]["events"] == 0 and empty["rare_events"]["event_head"].shape == (0, 4)
        assert _eq(empty["rare_events"]["game_second"], want["rare_events"]["game_second"])
        assert _eq(empty["rare_events"]["strategy_second"], want["rare_events"]["strategy_second"])
        for name in NAMES:
            assert _eq(empty["game_stats"][name], want["game_stats"][name]), name


def test_hip_chunks_and_split_calls_keep_the_order(eng, sparse_want):
    eng.set_option("chunk_bytes", 1 << 20)  # the smallest workspace: several chunks per call, the running base carries over
    try:
        chunked = _sparse(eng)
        assert eng.timing()["play_launches"] >= 2
        dense = _sparse(eng, thresholds=(2 ** 31 - 1,))
        assert eng.timing()["play_launches"] >= 2
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    _same(chunked, sparse_want)
    whole_dense = _sparse(eng, thresholds=(2 ** 31 - 1,))
    assert whole_dense["rare_events"]["events"] == whole_dense["game_stats"]["game_counts"][gs.COMPLETED] > 1000
    _same(dense, whole_dense)
    _same(whole_dense, StubEngine().tournament_rare_events(_table(64), 4, 9, 100, 700, max_rounds=12, thresholds=(2 ** 31 - 1,)))
    for thresholds, whole in ((SPARSE["thresholds"], sparse_want), ((2 ** 31 - 1,), whole_dense)):
        cuts = (100, 333, 334, 700)
        parts = [_sparse(eng, a, b, thresholds=thresholds) for a, b in zip(cuts, cuts[1:])]
        head, seats = rev.concat_events([(p["rare_events"]["event_head"], p["rare_events"]["event_seats"]) for p in parts],
                                        [a - 100 for a in cuts[:3]])
        assert np.array_equal(head, whole["rare_events"]["event_head"]) and np.array_equal(seats, whole["rare_events"]["event_seats"])
        merged = rev.RareEventSummary.from_engine(parts[0], 4).merge(rev.RareEventSummary.from_engine(parts[1], 4)).merge(
            rev.RareEventSummary.from_engine(parts[2], 4))
        assert _eq(merged.game_second, whole["rare_events"]["game_second"])
        assert _eq(merged.strategy_second, whole["rare_events"]["strategy_second"])
        for name in NAMES:
            assert _eq(merged.stats.to_arrays()[name], whole["game_stats"][name]), name


def test_hip_forced_second_score_spills(eng):
    t = _table(64)
    kw = dict(max_rounds=40, target_score=4000, rare_target_score=3000, thresholds=(200,))
    want = eng.tournament_rare_events(t, 2, 5, 0, 300, **kw)
    assert want["spilled"] == 0
    _same(want, StubEngine().tournament_rare_events(t, 2, 5, 0, 300, **kw))
    eng.set_option("game_stats_window", 3)  # second scores >= 150 points all go through the spill list (kind 3)
    try:
        spilled = eng.tournament_rare_events(t, 2, 5, 0, 300, **kw)
        tiny = eng.tournament_rare_events(t, 2, 5, 0, 300, spill_capacity=1, event_capacity=1, **kw)  # both lists short at once
    finally:
        eng.set_option("game_stats_window", 0)
    base = eng.tournament_game_stats(t, 2, 5, 0, 300, max_rounds=40, target_score=4000, rare_target_score=3000)
    assert base["spilled"] == 0
    assert spilled["spilled"] > 1000 and tiny["spilled"] == spilled["spilled"] and tiny["attempts"] == 2
    _same(spilled, want)
    _same(tiny, want)


def test_hip_event_capacity_one_short(eng, sparse_want):
    n = sparse_want["rare_events"]["events"]
    with pytest.raises(FarkleHipError) as err:
        _sparse(eng, event_capacity=n - 1, retry=False)
    assert err.value.code == FK_ERR_ARG and err.value.events_needed == n
    exact = _sparse(eng, event_capacity=n, retry=False)
    assert exact["attempts"] == 1
    _same(exact, sparse_want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_fixture_cases_equal_the_reference(eng, case):
    check_case(case, eng)
