"""RNG diagnostics, matchup family, on the MI355X: the key post-pass's records bit for bit against the oracle's rows (chunk
boundaries, split calls, every seat count of the fixture), the device reduce against the host statement (forced digest-collision
runs included), the reference's own rows and report end to end, and a 10^6-game table."""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu
from test_rng_matchups_cpu import case_table, cell_overrides, cell_records, check_case, check_games, rm_lags, select_case

from farkle_ii_amd import rng_matchups as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _odd_ids(S: int) -> np.ndarray:
    """Unique IDs whose order is NOT the table order: the tuple is sorted by ID."""
    return ((np.arange(S, dtype=np.int64) * 7919 + 13) % 1_000_003 - 400_000).astype(np.int32)


def _same_records(a: dict, b: dict) -> None:
    for key in ("digest", "seats", "rounds"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def _same_reduce(got: dict, want: dict, ids: np.ndarray, cap) -> None:
    for key in ("observations", "candidate_groups", "eligible_groups"):
        assert got[key] == want[key], key
    assert np.array_equal(got["histogram"], want["histogram"])
    g = rm.MatchupGroups.from_reduce(got, ids, 12, cap)
    w = rm.MatchupGroups.from_reduce(want, ids, 12, cap)
    for key in ("priority", "group_id", "participants", "count", "sums"):
        assert np.array_equal(getattr(g, key), getattr(w, key)), key


@pytest.mark.parametrize("index", [0, 1, 2])
def test_hip_fixture_cases_equal_the_reference(eng, index):
    case = gu.load("rng_matchup_vectors.json")["cases"][index]
    reduced = []
    for cell in case["cells"]:
        res, ids = cell_records(eng, case, cell)
        check_games(case, cell, res["matchups"], ids)
        reduced.append(eng.matchup_reduce(res["matchups"], cell["k"], rm_lags(), rm.effective_cap(case["rng_max_matchup_groups"])))
    rows, report = select_case(case, reduced)
    check_case(case, rows, report)


def test_hip_records_equal_the_oracle_across_chunks_and_calls(eng):
    from matchup_engine_stub import Engine as StubEngine

    from bench import grid64
    from tools.time_config import table_for

    stub = StubEngine()
    t64 = grid64()
    ids64 = _odd_ids(64)
    lags = (1, 2, 7)
    want = stub.tournament_matchups(t64, 2, 42, 100, 400, lags, ids64, 12, shuffles_per_batch=50)
    whole = eng.tournament_matchups(t64, 2, 42, 100, 400, lags, ids64, 12, shuffles_per_batch=50)
    _same_records(whole["matchups"], want["matchups"])
    for key in ("tally", "lag_sums", "lag_head", "lag_tail"):  # the strategy family is tournament_lags' own
        assert np.array_equal(whole[key], want[key]), key
    eng.set_option("chunk_bytes", 1 << 20)  # the smallest workspace: several chunks per call
    try:
        chunked = eng.tournament_matchups(t64, 2, 42, 100, 400, lags, ids64, 12, shuffles_per_batch=50)
        assert eng.timing()["play_launches"] >= 2
        t5160 = table_for(5160)
        ids = _odd_ids(5160)
        small = eng.tournament_matchups(t5160, 4, 3, 10, 30, (1, 3), ids, 12)
        assert eng.timing()["play_launches"] >= 5
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    _same_records(chunked["matchups"], want["matchups"])
    _same_records(small["matchups"], stub.tournament_matchups(t5160, 4, 3, 10, 30, (1, 3), ids, 12)["matchups"])
    # calls cut anywhere concatenate to the whole; eight and twelve seats (hot / cold kernels), max_players beyond twelve
    for k, n_sh, mp in ((8, 12, 12), (12, 6, 12), (3, 9, 31)):
        table = t5160[:5160 - 5160 % k]
        idk = ids[:len(table)]
        want = stub.tournament_matchups(table, k, 0, 0, n_sh, (1,), idk, mp)["matchups"]
        parts = [eng.tournament_matchups(table, k, 0, b, e, (1,), idk, mp)["matchups"] for b, e in ((0, 1), (1, 4), (4, n_sh))]
        _same_records(rm.concat_records(parts, k), want)


def test_hip_reduce_equals_the_host_statement_with_forced_collisions(eng):
    from bench import grid64

    t64 = grid64()
    ids = _odd_ids(64)
    rec = eng.tournament_matchups(t64, 2, 9, 0, 600, (1,), ids, 12)["matchups"]  # 19 200 games over 2 016 tuples
    for lags, cap in (((1, 2, 5), None), ((1, 2, 5), 40), ((3,), 7), ((1,), 1)):
        _same_reduce(eng.matchup_reduce(rec, 2, lags, cap), rm.host_reduce(rec, 2, lags, cap), ids, cap)
    # the sort key masked down to a few bits: runs of equal key hold many tuples, and groups must still be exact
    try:
        for mask in (0, 0xF, 0xFF00000000000000):
            eng.set_option("matchup_sort_key_mask", mask)
            _same_reduce(eng.matchup_reduce(rec, 2, (1, 2, 5), 25), rm.host_reduce(rec, 2, (1, 2, 5), 25), ids, 25)
    finally:
        eng.set_option("matchup_sort_key_mask", -1)
    # k = 4 on a larger table: almost every group a singleton
    from tools.time_config import table_for

    t = table_for(5160)
    ids = _odd_ids(5160)
    rec4 = eng.tournament_matchups(t, 4, 1, 0, 40, (1,), ids, 12)["matchups"]
    _same_reduce(eng.matchup_reduce(rec4, 4, (1,), None), rm.host_reduce(rec4, 4, (1,), None), ids, None)
    empty = eng.matchup_reduce({"digest": rec["digest"][:0], "seats": rec["seats"][:0], "rounds": rec["rounds"][:0]}, 2, (1,), 5)
    assert empty["observations"] == 0 and empty["candidate_groups"] == 0 and len(empty["count"]) == 0


def test_hip_million_game_table_with_cap_1000(eng):
    """k = 2 over 80 strategies: 40 games per shuffle, 25 000 shuffles = 10^6 games in 3 160 groups of ~316 observations."""
    from tools.time_config import table_for

    t = table_for(80)
    ids = _odd_ids(80)
    res = eng.tournament_matchups(t, 2, 3, 0, 25_000, (1, 2, 5), ids, 12)
    rec = res["matchups"]
    assert len(rec["digest"]) == 1_000_000
    sid = ids[rec["seats"].astype(np.int64)]
    assert np.all(sid[:, 0] < sid[:, 1])
    assert np.array_equal(rec["digest"], rm.digests(2, sid, 12))
    got = eng.matchup_reduce(rec, 2, (1, 2, 5), 1000)
    want = rm.host_reduce(rec, 2, (1, 2, 5), 1000)
    _same_reduce(got, want, ids, 1000)
    assert got["candidate_groups"] == 3160 and len(rm.MatchupGroups.from_reduce(got, ids, 12, 1000).count) == 1000


def test_hip_matchup_request_validation(eng):
    from bench import grid64

    from farkle_ii_amd.backend import FarkleHipError

    t = grid64()
    with pytest.raises(FarkleHipError):
        eng.tournament_matchups(t, 2, 1, 0, 4, (1,), np.arange(64), 1)  # max_players < k
    with pytest.raises(FarkleHipError):
        eng.tournament_matchups(t, 2, 1, 0, 4, (1,), np.arange(64), 32)  # beyond one BLAKE2b block
    with pytest.raises(FarkleHipError):
        eng.tournament_matchups(t, 2, 1, 0, 4, (2, 1), np.arange(64), 12)
    with pytest.raises(ValueError):
        eng.tournament_matchups(t, 2, 1, 0, 4, (1,), np.zeros(64), 12)  # IDs must be unique
