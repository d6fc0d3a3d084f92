"""RNG diagnostics, matchup family, on the CPU: the digest restatement against ``hashlib``, and the host statement of the rule
(records, reduce, selection across player counts, rows, report) against `tests/golden/rng_matchup_vectors.json` — produced by the
reference's OWN ``_extract_batch_arrays`` / ``_count_records`` / ``_observation_records`` / ``_priority`` / ``_OnlineMetric`` /
``_rows_for_online_group`` over rows it simulated (`tools/gen_rng_matchup_golden.py`)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import golden_util as gu  # noqa: E402
from matchup_engine_stub import Engine as StubEngine  # noqa: E402

from farkle_ii_amd import rng_matchups as rm  # noqa: E402
from farkle_ii_amd.backend import make_overrides  # noqa: E402
from farkle_ii_amd.strategies import STRATEGY_DTYPE  # noqa: E402


def case_table(case):
    table = gu.strategies_from_tuples(case["strategies"], STRATEGY_DTYPE)
    return table, np.asarray(table["strategy_id"], dtype=np.int32)


def cell_overrides(cell):
    return make_overrides((o[0], o[2], o[3], o[1], o[4]) for o in cell["overrides"]) if cell["overrides"] else None


def cell_records(eng, case, cell):
    table, ids = case_table(case)
    res = eng.tournament_matchups(table, cell["k"], case["root_seed"], 0, cell["n_shuffles"], rm_lags(), ids, case["max_players"],
                                  target_score=case["target_score"], max_rounds=case["max_rounds"], overrides=cell_overrides(cell))
    return res, ids


def rm_lags():
    return tuple(gu.load("rng_matchup_vectors.json")["lags"])


def check_games(case, cell, records, ids):
    """Per game, in coordinate order: (k, sorted IDs, digest) == the reference's."""
    k = cell["k"]
    seats = np.asarray(records["seats"]).reshape(-1, k)
    got = [[k, [int(v) for v in ids[seats[i].astype(np.int64)]], str(int(records["digest"][i]))] for i in range(len(seats))]
    assert got == cell["games"]


def select_case(case, reduced):
    """Per-k reduce results -> the root's rows and report."""
    lags = rm_lags()
    _, ids = case_table(case)
    cap = rm.effective_cap(case["rng_max_matchup_groups"])
    groups = [rm.MatchupGroups.from_reduce(r, ids, case["max_players"], cap) for r in reduced]
    strategies = [rm.StrategyFamily(c["k"], len(ids), c["n_shuffles"]) for c in case["cells"]]
    return rm.select(groups, strategies, lags, cap, case["rng_diagnostic_partitions"])


def check_case(case, rows, report):
    assert report == case["report"]
    key = lambda r: (r["n_players"], r["matchup_id"], r["participant_strategy_ids"], r["lag"])  # noqa: E731
    assert rows == sorted(case["rows"], key=key)  # floats included


def test_digest_restatement_equals_hashlib():
    rng = np.random.default_rng(7)
    for k in range(1, 13):
        ids = np.sort(rng.integers(-(1 << 31), 1 << 31, size=(17, k)), axis=1).astype(np.int32)
        for mp in (k, 12, 31) if k <= 12 else (k, 31):
            want = [rm.digest_hashlib(k, row, mp) for row in ids]
            assert [int(v) for v in rm.digests(k, ids, mp)] == want, (k, mp)
    doc = gu.load("rng_matchup_vectors.json")
    for case in doc["cases"]:
        for cell in case["cells"]:
            for k, sorted_ids, digest in cell["games"][:50]:
                assert rm.digest_hashlib(k, sorted_ids, case["max_players"]) == int(digest)


@pytest.mark.parametrize("index", [0, 1, 2])
def test_host_records_reduce_and_selection_equal_the_reference(index):
    case = gu.load("rng_matchup_vectors.json")["cases"][index]
    eng = StubEngine()
    reduced = []
    for cell in case["cells"]:
        res, ids = cell_records(eng, case, cell)
        check_games(case, cell, res["matchups"], ids)
        reduced.append(eng.matchup_reduce(res["matchups"], cell["k"], rm_lags(), rm.effective_cap(case["rng_max_matchup_groups"])))
    rows, report = select_case(case, reduced)
    check_case(case, rows, report)
    if index == 1:
        assert report["completeness_status"] == "blocked_by_cap" and report["priority_cutoff"] is not None
    if index == 2:
        assert rows == [] and report["eligible_matchup_groups"] == 0


def test_split_ranges_concatenate_to_the_whole():
    case = gu.load("rng_matchup_vectors.json")["cases"][0]
    cell = case["cells"][0]
    table, ids = case_table(case)
    eng = StubEngine()
    kw = dict(target_score=case["target_score"], max_rounds=case["max_rounds"], overrides=cell_overrides(cell))
    parts = [eng.tournament_matchups(table, cell["k"], case["root_seed"], b, e, rm_lags(), ids, 12, **kw)["matchups"]
             for b, e in ((0, 7), (7, 8), (8, cell["n_shuffles"]))]
    check_games(case, cell, rm.concat_records(parts, cell["k"]), ids)


def test_priority_ties_and_collisions_in_the_host_reduce():
    """Groups are tuples, not digests: two tuples forced onto one digest stay two groups, each series in record order."""
    k = 2
    seats = np.array([[0, 1], [2, 3], [0, 1], [2, 3], [0, 1], [2, 3], [0, 1]], dtype=np.uint16)
    rounds = np.array([5, 9, 6, 8, 7, 7, 9], dtype=np.uint16)
    rec = {"digest": np.full(7, 42, dtype=np.uint64), "seats": seats, "rounds": rounds}
    res = rm.host_reduce(rec, k, (1,), None)
    assert res["candidate_groups"] == 2 and res["eligible_groups"] == 2
    by = {tuple(int(v) for v in s): (int(c), x) for s, c, x in zip(res["seats"], res["count"], res["sums"])}
    assert by[(0, 1)][0] == 4 and by[(0, 1)][1][0].tolist() == [3, 5 + 6 + 7, 6 + 7 + 9, 25 + 36 + 49, 36 + 49 + 81, 30 + 42 + 63]
    assert by[(2, 3)][1][0].tolist() == [2, 17, 15, 145, 113, 128]
    # ties on the 64-bit priority: the cut keeps every tied group; MatchupGroups breaks the tie by the participants
    capped = rm.host_reduce(rec, k, (1,), 1)
    assert len(capped["count"]) == 2
    g = rm.MatchupGroups.from_reduce(capped, np.array([10, 11, 12, 13], dtype=np.int32), 12, 1)
    assert g.participants[:, :2].tolist() == [[10, 11]]


def test_histogram_labels_and_bins_follow_the_reference():
    counts = np.array([1, 2, 3, 4, 5, 6, 10, 100, 40000])
    bins = rm.histogram_bin(counts, 3)
    assert bins.tolist() == [1, 2, 3, 4, 4, 5, 6, 9, 18]
    assert [rm.histogram_label(int(b), 3) for b in bins[:6]] == ["1", "2", "3-3", "4-5", "4-5", "6-9"]
    assert rm.effective_cap(None) == 100_000 and rm.effective_cap(0) is None and rm.effective_cap(-3) is None and rm.effective_cap(7) == 7
