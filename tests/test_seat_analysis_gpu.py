"""The seat-analysis stage on the MI355X: ``fk_tournament_run_seat_counts`` against the host statement over the oracle's rows, exact
equality everywhere — per-seat counts at every seat count up to sixteen with a ragged last batch and safety-limit games, workspace
chunks that cut batches, the mirrored pairs of one long pair (segments across wave and workgroup boundaries), of a tiny table (long
interleaved segments) and of many short ones, the capacity convention, split calls, the refusals, every fixture case end to end,
and the tally of ``fk_tournament_run``."""
from __future__ import annotations

import numpy as np
import pytest

from seat_analysis_engine_stub import Engine as StubEngine
from test_seat_analysis_cpu import CASES, case_table, cell_result, check_case

from farkle_ii_amd import seat_analysis as sa
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError, make_overrides

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _table(S: int):
    """Up to twelve strategies: the fixture's grid (every one banks, so games complete); beyond: the benchmark grids."""
    if S <= 12:
        return case_table(CASES[0])[0][:S].copy()
    from tools.time_config import table_for

    return table_for(64)[:S].copy() if S <= 64 else table_for(S)


def _ids(S: int) -> np.ndarray:
    """Unique IDs whose order is not the table's: the pairing is by ID rank, the outputs name table indices."""
    return ((np.arange(S, dtype=np.int64) * 37 + 11) % 257).astype(np.int32) if S <= 257 else np.arange(S, dtype=np.int32)[::-1].copy()


def _same_counts(got: dict, want: dict) -> None:
    assert got["seat_counts"].shape == want["seat_counts"].shape
    assert np.array_equal(got["seat_counts"], want["seat_counts"])
    assert np.array_equal(got["tally"], want["tally"])


def _same_pairs(got: dict, want: dict) -> None:
    assert np.array_equal(got["pair_index"], want["pair_index"])
    assert np.array_equal(got["pair_sums"], want["pair_sums"])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 12])
def test_hip_seat_counts_equal_the_host_statement(eng, k):
    t = _table(12)
    ov = make_overrides([(42, 3, 0, k, 2), (42, 17, 0, k, 1), (42, 39, 12 // k - 1, k, 3)])  # safety-limit games, one in the ragged batch
    kw = dict(shuffles_per_batch=16, overrides=ov, target_score=3000)
    want = StubEngine().tournament_seat_counts(t, k, 42, 0, 40, **kw)
    got = eng.tournament_seat_counts(t, k, 42, 0, 40, **kw)
    _same_counts(got, want)
    c = got["seat_counts"]
    assert c.shape == (3, 12, k, 3) and c[..., sa.SAFETY].sum() >= 2 * k
    assert np.array_equal((c[..., sa.COMPLETED] + c[..., sa.SAFETY]).sum(axis=2), np.repeat([[16], [16], [8]], 12, axis=1))  # one seat per shuffle
    assert np.array_equal(got["tally"], eng.tournament(t, k, 42, 0, 40, **kw)["tally"])  # the tally of fk_tournament_run, bit for bit
    if k > 2:
        assert (c[..., sa.COMPLETED] + c[..., sa.SAFETY] == 0).any()  # cells the reference would not emit


def test_hip_seat_counts_sixteen_seats_and_the_refusal_beyond(eng):
    t = _table(16)
    ov = make_overrides([(7, 5, 0, 16, 2)])
    want = StubEngine().tournament_seat_counts(t, 16, 7, 0, 40, shuffles_per_batch=16, overrides=ov, target_score=3000)
    _same_counts(eng.tournament_seat_counts(t, 16, 7, 0, 40, shuffles_per_batch=16, overrides=ov, target_score=3000), want)
    with pytest.raises(FarkleHipError) as err:
        eng.tournament_seat_counts(_table(34), 17, 7, 0, 4, target_score=3000)
    assert err.value.code == FK_ERR_ARG


def test_hip_seat_counts_when_chunks_cut_batches(eng):
    t = _table(64)
    kw = dict(shuffles_per_batch=32, max_rounds=12)  # many safety-limit games; the call's first batch is batch 1 of the run
    want = StubEngine().tournament_seat_counts(t, 2, 9, 32, 332, **kw)
    assert want["seat_counts"][..., sa.SAFETY].sum() > 0 and len(want["seat_counts"]) == 10
    _same_counts(eng.tournament_seat_counts(t, 2, 9, 32, 332, **kw), want)
    eng.set_option("chunk_bytes", 1 << 20)  # the smallest workspace: several chunks per call, cutting batches
    try:
        chunked = eng.tournament_seat_counts(t, 2, 9, 32, 332, strategy_ids=_ids(64), want_mirrored=True, **kw)
        launches = eng.timing()["play_launches"]
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    assert launches >= 2
    _same_counts(chunked, want)
    _same_pairs(chunked, eng.tournament_seat_counts(t, 2, 9, 32, 332, strategy_ids=_ids(64), want_mirrored=True, **kw))


MIRRORED = {
    # one pair: segments of 300 / 300 / 100 games cross wave and workgroup boundaries
    "one_pair": dict(S=2, n_sh=700, spb=300, ov=[(3, 5, 0, 2, 1), (3, 311, 0, 2, 2), (3, 650, 0, 2, 1)]),
    # six pairs, segments of about five games, orientations interleaved
    "tiny_table": dict(S=4, n_sh=64, spb=16, ov=[(3, 2, 0, 2, 1), (3, 20, 1, 2, 2), (3, 63, 0, 2, 1)]),
    # 2 016 possible pairs, segments of 0 - 3 games
    "grid64": dict(S=64, n_sh=96, spb=32, ov=[(3, 0, 0, 2, 1), (3, 40, 31, 2, 2), (3, 95, 7, 2, 1)]),
}


def _mirrored(e, name, begin=0, end=None, **extra):
    m = MIRRORED[name]
    return e.tournament_seat_counts(_table(m["S"]), 2, 3, begin, m["n_sh"] if end is None else end, shuffles_per_batch=m["spb"],
                                    overrides=make_overrides(m["ov"]), target_score=3000, strategy_ids=_ids(m["S"]), want_mirrored=True, **extra)


@pytest.fixture(scope="module")
def mirrored_want():
    return {name: _mirrored(StubEngine(), name) for name in MIRRORED}


@pytest.mark.parametrize("name", list(MIRRORED))
def test_hip_mirrored_pairs_equal_the_two_queue_loop(eng, mirrored_want, name):
    want = mirrored_want[name]
    got = _mirrored(eng, name)
    _same_counts(got, want)
    _same_pairs(got, want)
    sums = got["pair_sums"]
    assert sums[:, 3].sum() >= len(MIRRORED[name]["ov"])  # every safety-limit game is in its pair's row
    assert (sums[:, 2] + sums[:, 3]).sum() == MIRRORED[name]["n_sh"] * (MIRRORED[name]["S"] // 2)  # and every game in one row
    if name == "one_pair":
        assert len(sums) == 1 and sums[0, 0] > 250  # three long segments
    if name == "grid64":
        assert len(sums) > 1000 and (sums[:, 0] == 0).any() and (sums[:, 0] > 0).any()


def test_hip_pair_capacity_one_short_reports_the_count(eng, mirrored_want):
    n = len(mirrored_want["grid64"]["pair_sums"])
    with pytest.raises(FarkleHipError) as err:
        _mirrored(eng, "grid64", pair_capacity=n - 1, retry=False)
    assert err.value.code == FK_ERR_ARG and err.value.pairs_needed == n
    again = _mirrored(eng, "grid64", pair_capacity=n - 1)  # once more with the reported room
    assert again["attempts"] == 2
    _same_pairs(again, mirrored_want["grid64"])
    exact = _mirrored(eng, "grid64", pair_capacity=n)
    assert exact["attempts"] == 1
    _same_pairs(exact, mirrored_want["grid64"])


@pytest.mark.parametrize("name", ["one_pair", "grid64"])
def test_hip_split_at_a_batch_boundary_and_merged_is_one_call(eng, mirrored_want, name):
    m = MIRRORED[name]
    ids = _ids(m["S"])
    cut = m["spb"] * (2 if name == "one_pair" else 1)
    parts = [(sa.SeatCounts.from_engine(r, 2, a // m["spb"]), sa.MirroredPairs.from_engine(r, ids))
             for a, r in ((0, _mirrored(eng, name, 0, cut)), (cut, _mirrored(eng, name, cut, m["n_sh"])))]
    counts, pairs = parts[1][0].merge(parts[0][0]), parts[0][1].merge(parts[1][1])
    whole = sa.MirroredPairs.from_engine(mirrored_want[name], ids)
    assert np.array_equal(counts.counts, mirrored_want[name]["seat_counts"])
    assert np.array_equal(pairs.ids, whole.ids) and np.array_equal(pairs.sums, whole.sums)


def test_hip_refuses_an_unaligned_begin_and_pairs_beyond_two_seats(eng):
    with pytest.raises(FarkleHipError) as err:
        _mirrored(eng, "tiny_table", 8, 64)
    assert err.value.code == FK_ERR_ARG and "multiple of shuffles_per_batch" in str(err.value)
    # (the counts alone may start anywhere: batches are numbered from the call's first shuffle, as the tally's are)
    t = _table(4)
    got = eng.tournament_seat_counts(t, 2, 3, 8, 64, shuffles_per_batch=16, target_score=3000)
    _same_counts(got, StubEngine().tournament_seat_counts(t, 2, 3, 8, 64, shuffles_per_batch=16, target_score=3000))
    with pytest.raises(FarkleHipError) as err:
        eng.tournament_seat_counts(_table(12), 3, 3, 0, 16, shuffles_per_batch=16, strategy_ids=_ids(12), want_mirrored=True)
    assert err.value.code == FK_ERR_ARG and "k = 2 only" in str(err.value)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_fixture_cases_equal_the_reference(eng, case):
    check_case(case, [cell_result(eng, case, cell) for cell in case["cells"]])
