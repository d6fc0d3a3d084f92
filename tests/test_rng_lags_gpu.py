"""fk_tournament_run_lags on the MI355X: the reference's own RNG-diagnostics rows (strategy family), the oracle-backed statement of
the rule on larger tables, chunk carries shorter than the largest lag, and range merges."""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu
from test_rng_lags_cpu import case_inputs, check_against_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


@pytest.mark.parametrize("index", [0, 1])
def test_hip_lag_statistics_equal_the_reference_rows(eng, index):
    doc = gu.load("rng_lag_vectors.json")
    case, lags = doc["cases"][index], doc["lags"]
    table, ov = case_inputs(case)
    res = eng.tournament_lags(table, case["k"], case["root_seed"], 0, case["n_shuffles"], lags, target_score=case["target_score"],
                              max_rounds=case["max_rounds"], overrides=ov)
    check_against_reference(case, lags, res)


def _same(a: dict, b: dict) -> None:
    for key in ("tally", "lag_sums", "lag_head", "lag_tail"):
        assert np.array_equal(a[key], b[key]), key


def test_hip_equals_the_oracle_statement_on_larger_tables_and_across_chunks(eng):
    from oracle_engine_stub import Engine as StubEngine

    from bench import grid64
    from farkle_ii_amd.rng_lags import LagSummary
    from tools.time_config import table_for

    stub = StubEngine()
    t64 = grid64()
    # one batch on the 64-strategy grid: the LDS-tally launch (result records are written beside it for the value matrix)
    lags = (1, 2, 7)
    want = stub.tournament_lags(t64, 2, 42, 100, 700, lags)
    _same(eng.tournament_lags(t64, 2, 42, 100, 700, lags), want)
    t5160 = table_for(5160)
    eng.set_option("chunk_bytes", 1 << 20)  # the smallest workspace: three chunks here, four-shuffle chunks on the 5 160 grid
    try:
        got = eng.tournament_lags(t64, 2, 42, 100, 700, lags, shuffles_per_batch=50)
        assert eng.timing()["play_launches"] >= 3
        # chunks SHORTER than the largest lag: the carry rows of a chunk come from several earlier chunks
        small = eng.tournament_lags(t5160, 4, 3, 10, 40, (1, 3, 6))
        assert eng.timing()["play_launches"] >= 7
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    _same(got, stub.tournament_lags(t64, 2, 42, 100, 700, lags, shuffles_per_batch=50))
    _same(small, stub.tournament_lags(t5160, 4, 3, 10, 40, (1, 3, 6)))
    # the 5 160-strategy grid at four and eight seats (hot / cold kernels), and a range cut into calls that merge back
    for k, n_sh in ((4, 40), (8, 24)):
        table = t5160[:5160 - 5160 % k]
        want = stub.tournament_lags(table, k, 0, 0, n_sh, (1, 3))
        whole = eng.tournament_lags(table, k, 0, 0, n_sh, (1, 3))
        _same(whole, want)
        merged = None
        for b, e in ((0, 2), (2, 3), (3, n_sh - 9), (n_sh - 9, n_sh)):
            part = LagSummary.from_engine(eng.tournament_lags(table, k, 0, b, e, (1, 3)), (1, 3))
            merged = part if merged is None else merged.merge(part)
        assert np.array_equal(merged.sums, whole["lag_sums"]) and np.array_equal(merged.tail, whole["lag_tail"])


def test_hip_lags_at_and_beyond_the_series_length(eng):
    """70 shuffles with lags 69 (one pair per strategy), 70, 71 and 65 535 (none): the sums kernel's loop starts at
    ``max(r0, valid_from + lag)`` beyond the chunk, the carry is 65 535 rows deep and head / tail are the whole range.

    A shuffle of the 64-strategy grid at two seats takes 3 840 bytes of workspace, so its 70 shuffles fit one chunk even of the
    smallest workspace (1 MiB holds 273); that run is compared all the same, and the carry across chunks is driven by the first
    1 024 strategies of the default grid, whose 70 shuffles take at least five chunks there."""
    from oracle_engine_stub import Engine as StubEngine

    from bench import grid64
    from farkle_ii_amd.rng_lags import LagSummary
    from test_rng_lags_cpu import BEYOND_LAGS as lags, BEYOND_SHUFFLES as n_sh
    from tools.time_config import table_for

    stub = StubEngine()
    t64, t1024 = grid64(), table_for(1024)
    want = stub.tournament_lags(t64, 2, 42, 0, n_sh, lags)
    want_wide = stub.tournament_lags(t1024, 2, 5, 0, n_sh, lags)
    for w in (want, want_wide):
        assert np.all(w["lag_sums"][:, 1, 0] == 1) and not w["lag_sums"][:, 2:].any() and len(w["lag_head"]) == n_sh
    _same(eng.tournament_lags(t64, 2, 42, 0, n_sh, lags), want)
    _same(eng.tournament_lags(t1024, 2, 5, 0, n_sh, lags), want_wide)
    eng.set_option("chunk_bytes", 1 << 20)
    try:
        small = eng.tournament_lags(t64, 2, 42, 0, n_sh, lags)
        print("play launches, 64 strategies:", eng.timing()["play_launches"])
        wide = eng.tournament_lags(t1024, 2, 5, 0, n_sh, lags)
        print("play launches, 1 024 strategies:", eng.timing()["play_launches"])
        assert eng.timing()["play_launches"] >= 3
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    _same(small, want)
    _same(wide, want_wide)
    for table, seed, w in ((t64, 42, want), (t1024, 5, want_wide)):  # two calls, each shorter than every lag but the first
        a, b = (LagSummary.from_engine(eng.tournament_lags(table, 2, seed, lo, hi, lags), lags) for lo, hi in ((0, 30), (30, n_sh)))
        merged = a.merge(b)
        assert merged.n == n_sh and np.array_equal(merged.sums, w["lag_sums"])
        assert np.array_equal(merged.head, w["lag_head"]) and np.array_equal(merged.tail, w["lag_tail"])


def test_lag_request_validation(eng):
    from bench import grid64
    from farkle_ii_amd.backend import FarkleHipError

    for bad in ((), (0, 1), (2, 2), (3, 1), tuple(range(1, 18))):
        with pytest.raises(FarkleHipError):
            eng.tournament_lags(grid64(), 2, 42, 0, 10, bad)
    with pytest.raises(FarkleHipError):
        eng.tournament_lags(grid64(), 2, 42, 0, 10, (1,), max_rounds=40_000)
    res = eng.tournament_lags(grid64(), 2, 42, 5, 5, (1, 4))  # empty range
    assert res["n_shuffles"] == 0 and not res["lag_sums"].any() and len(res["lag_head"]) == 0
