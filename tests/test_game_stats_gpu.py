"""The game-stats stage on the MI355X: ``fk_tournament_run_game_stats`` against the host statement over the oracle's rows (every
seat count up to twelve, chunk boundaries, split calls, safety-limit games, the all-player arrays of the same launch), the forced
spill path, a large max_rounds, every fixture case end to end, and two large launches (conservation, additivity)."""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu
from game_stats_engine_stub import Engine as StubEngine
from test_game_stats_cpu import CASES, case_table, cell_summary, check_case

from farkle_ii_amd import game_stats as gs
from farkle_ii_amd.backend import make_overrides

pytestmark = pytest.mark.gpu

NAMES = ("strategy_counts", "strategy_rounds", "strategy_runner", "strategy_spread", "game_counts", "game_rounds", "game_runner")


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _eq(a, b) -> bool:
    """Histograms are equal when they agree bin for bin (the shorter one is zero beyond its end)."""
    a, b = np.asarray(a), np.asarray(b)
    n = max(a.shape[-1], b.shape[-1])
    pad = lambda x: gs._add_padded(x, np.zeros(x.shape[:-1] + (n,), np.int64))  # noqa: E731
    return np.array_equal(pad(a), pad(b))


def _same(got: dict, want: dict) -> None:
    for name in NAMES:
        assert _eq(got["game_stats"][name], want["game_stats"][name]), name
    assert np.array_equal(got["tally"], want["tally"])


def _table(S: int):
    from tools.time_config import table_for

    return table_for(S)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_hip_equals_the_host_statement_over_oracle_rows(eng, k):
    t = _table(120)
    ov = make_overrides([(42, 3, 0, k, 2), (42, 7, 1, k, 1), (42, 11, 2, k, 3)])  # safety-limit games
    kw = dict(shuffles_per_batch=16, overrides=ov, rare_target_score=2000, target_score=3000)
    want = StubEngine().tournament_game_stats(t, k, 42, 0, 40, **kw)
    got = eng.tournament_game_stats(t, k, 42, 0, 40, **kw)
    _same(got, want)
    assert got["game_stats"]["game_counts"][gs.SAFETY] >= 2
    if k in (2, 5):  # the all-player arrays ride on the same launch
        both = eng.tournament_game_stats(t, k, 42, 0, 40, want_seat_stats=True, **kw)
        ap = eng.tournament(t, k, 42, 0, 40, want_seat_stats=True, shuffles_per_batch=16, overrides=ov, target_score=3000)
        _same(both, want)
        assert np.array_equal(both["seat_stats"], ap["seat_stats"])
        assert both["seat_ratio_sums"].tobytes() == ap["seat_ratio_sums"].tobytes()


def test_hip_chunks_and_split_calls(eng):
    t = _table(64)
    want = StubEngine().tournament_game_stats(t, 4, 9, 100, 700, max_rounds=12)  # many safety-limit games
    assert want["game_stats"]["game_counts"][gs.SAFETY] > 0
    _same(eng.tournament_game_stats(t, 4, 9, 100, 700, max_rounds=12), want)
    eng.set_option("chunk_bytes", 1 << 20)  # the smallest workspace: several chunks per call
    try:
        chunked = eng.tournament_game_stats(t, 4, 9, 100, 700, max_rounds=12)
        assert eng.timing()["play_launches"] >= 2
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    _same(chunked, want)
    parts = [gs.GameStatsSummary.from_engine(eng.tournament_game_stats(t, 4, 9, a, b, max_rounds=12), 4)
             for a, b in ((100, 333), (333, 334), (334, 700))]
    merged = parts[0].merge(parts[1]).merge(parts[2]).to_arrays()
    for name in NAMES:
        assert _eq(merged[name], want["game_stats"][name]), name


def test_hip_forced_spill_gives_identical_results(eng):
    t = _table(64)
    want = eng.tournament_game_stats(t, 2, 5, 0, 300, max_rounds=40, target_score=4000)
    assert want["spilled"] == 0
    eng.set_option("game_stats_window", 3)  # n_rounds >= 3 and margins >= 150 points all go through the spill list
    try:
        spilled = eng.tournament_game_stats(t, 2, 5, 0, 300, max_rounds=40, target_score=4000)
        tiny = eng.tournament_game_stats(t, 2, 5, 0, 300, max_rounds=40, target_score=4000, spill_capacity=1)  # FK_ERR_ARG, then room
    finally:
        eng.set_option("game_stats_window", 0)
    assert spilled["spilled"] > 1000 and tiny["spilled"] == spilled["spilled"]
    _same(spilled, want)
    _same(tiny, want)


def test_hip_large_max_rounds(eng):
    t = _table(64)
    ov = make_overrides([(5, 1, 0, 2, 32767)])
    want = StubEngine().tournament_game_stats(t, 2, 5, 0, 50, max_rounds=5000, overrides=ov)
    got = eng.tournament_game_stats(t, 2, 5, 0, 50, max_rounds=5000, overrides=ov)
    assert got["game_stats"]["strategy_rounds"].shape == (64, 32768)
    _same(got, want)
    eng.set_option("game_stats_window", 4)
    try:
        _same(eng.tournament_game_stats(t, 2, 5, 0, 50, max_rounds=5000, overrides=ov), want)
    finally:
        eng.set_option("game_stats_window", 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_fixture_cases_equal_the_reference(eng, case):
    check_case(case, [cell_summary(eng, case, cell) for cell in case["cells"]])


def _conserved(g: dict, n_games: int, n_sh: int) -> None:
    c = g["strategy_counts"]
    assert np.all(c[:, gs.ATTEMPTED] == n_sh)  # one exposure per strategy per shuffle
    assert np.array_equal(c[:, gs.ATTEMPTED], c[:, gs.COMPLETED] + c[:, gs.SAFETY])
    assert np.array_equal(c[:, gs.ATTEMPTED], g["strategy_rounds"].sum(axis=1))
    assert np.array_equal(c[:, gs.COMPLETED], g["strategy_runner"].sum(axis=1))
    assert np.array_equal(c[:, gs.COMPLETED], g["strategy_spread"].sum(axis=1))
    gc = g["game_counts"]
    assert gc[gs.ATTEMPTED] == n_games == gc[gs.COMPLETED] + gc[gs.SAFETY] == g["game_rounds"].sum()
    assert g["game_runner"].sum() == gc[gs.COMPLETED]


@pytest.mark.parametrize("S,k,n_sh", [(64, 2, 312_500), (5160, 4, 3000)], ids=["1e7_k2", "config3_shape"])
def test_hip_large_launches_conserve_and_add(eng, S, k, n_sh):
    t = _table(S)
    whole = eng.tournament_game_stats(t, k, 11, 0, n_sh)
    _conserved(whole["game_stats"], n_sh * (S // k), n_sh)
    cut = n_sh // 3
    a = gs.GameStatsSummary.from_engine(eng.tournament_game_stats(t, k, 11, 0, cut), k)
    b = gs.GameStatsSummary.from_engine(eng.tournament_game_stats(t, k, 11, cut, n_sh), k)
    merged = b.merge(a).to_arrays()
    for name in NAMES:
        assert _eq(merged[name], whole["game_stats"][name]), name
    assert np.array_equal(whole["tally"].sum(axis=0), eng.tournament(t, k, 11, 0, n_sh)["tally"].sum(axis=0))
