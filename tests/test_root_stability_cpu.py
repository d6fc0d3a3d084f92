"""The two-root stability stage's bootstrap families on the CPU: the host estimate chain, the NumPy host statement, the seams and the
three frames against `tests/golden/root_stability_bootstrap_vectors.json` — the reference's OWN ``_scope_estimates``,
``_discrepancies``, ``_RootTopNRangeWriter`` / ``_JointDiscrepancyRangeWriter`` and their reductions over synthetic batch matrices
(`tools/gen_root_stability_golden.py`) — bit for bit, and the refusals.

The across-k score / mcse columns go through ``np.dot`` in the reference; their bits depend on the machine's BLAS kernel, so every
comparison with fixture bits FEEDS the fixture's recorded columns in, and ``across_k_estimates`` is checked against ``np.dot``
evaluated here on the same operands."""
from __future__ import annotations

import sys
from math import sqrt
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import root_stability_cases as rc  # noqa: E402
from root_stability_engine_stub import Engine as StubEngine  # noqa: E402

from farkle_ii_amd import root_stability as rs  # noqa: E402

REDUCIBLE = [c for c in rc.CASES if c["root_discrepancies"] is not None]


def test_fixture_has_the_three_cases_and_their_properties():
    assert [c["name"] for c in rc.CASES] == ["k234", "tied_pairs_one_batch", "all_invalid"]
    main, tied, invalid = rc.CASES
    assert [len(m["batch_ids"]) for m in main["matrices"]] == [13, 9, 2, 13, 9, 2] and main["top_n"] == 10
    maxima = np.concatenate([m for *_, m in rc.case_ranges(main)])
    assert maxima.shape == (64,) and len(np.unique(maxima)) == 64
    member = np.concatenate([t for _, _, t, _ in rc.case_ranges(tied)])
    assert member.shape == (64, 2, 96) and tied["top_n"] == 9
    assert np.all(np.sum(member[:, :, 0::2] != member[:, :, 1::2], axis=2) == 1)  # one split pair per (replicate, root) ...
    assert np.all(member[:, :, 0::2] >= member[:, :, 1::2])                       # ... and the lower id wins
    maxima = np.concatenate([m for *_, m in rc.case_ranges(invalid)])
    assert maxima.shape == (64,) and maxima.tobytes() == np.zeros(64).tobytes()
    assert invalid["reference_reduction_error"].startswith("TypeError")  # the reference's own reduction fails on this case


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_estimate_chain_matches_reference(case):
    cells = rc.case_cells(case)
    assert cells.strategies.tolist() == case["strategies"] and list(cells.roots) == case["roots"]
    kw = rc.case_kwargs(case)
    weights = rs.k_weights(kw["k_aggregation_method"], kw["declared_k_weights"], cells.required_k)
    assert [w.hex() for w in weights] == case["weights"]
    estimates, frame, joint = rc.case_joint(case, cells)
    S, n_k = len(cells.strategies), len(cells.required_k)
    for k in cells.required_k:
        for scope in estimates.scopes[:2]:
            got = estimates.by_k[k][scope]["batch_mcse"]
            assert got.shape == (S,) and [v.hex() for v in got.tolist()] == rc.expand(case["by_k"][str(k)][scope]["batch_mcse"])
    want = rc.decode(case["root_discrepancies"] or case["root_discrepancies_before_joint"])
    assert tuple(name for name, _ in want["schema"][:17]) == rs.DISCREPANCY_COLUMNS
    for name in rs.DISCREPANCY_COLUMNS:
        got = [v.hex() if isinstance(v, float) else v for v in frame[name]]
        expect = want["columns"][name]
        if name in ("k", "expected_mcse", "standardized_discrepancy"):  # pandas -> Arrow: None and NaN are nulls, k is a double
            got = [None if v is None or v == "nan" else (float(v).hex() if name == "k" else v) for v in got]
        assert len(got) == (n_k + 1) * S and got == expect, name
    assert joint.observed.shape == (n_k, S) and joint.expected_across.shape == (S,)


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_across_k_function_is_the_reference_expression(case):
    """``np.dot`` evaluated HERE on the same operands: what the reference gives on the machine that runs the test."""
    cells = rc.case_cells(case)
    weights = rc.case_weights(case)
    kw = rc.case_kwargs(case)
    estimates = rs.scope_estimates(cells, weights, kw["practical_delta_by_k"], kw["delta_across_k"])
    weight_array = np.asarray(weights, dtype=float)
    checked = 0
    for scope in estimates.scopes:
        values = np.stack([estimates.by_k[k][scope]["chance_delta"] for k in cells.required_k])
        errors = np.stack([estimates.by_k[k][scope]["batch_mcse"] for k in cells.required_k])
        for s in range(values.shape[1]):
            want_score = float(np.dot(weight_array, np.asarray([float(v) for v in values[:, s]], dtype=float)))
            want_mcse = float(sqrt(np.dot(weight_array * weight_array, np.asarray([float(v) ** 2 for v in errors[:, s]], dtype=float))))
            assert estimates.across[scope]["across_k_score"][s].tobytes() == np.float64(want_score).tobytes()
            assert estimates.across[scope]["across_k_mcse"][s].tobytes() == np.float64(want_mcse).tobytes()
            checked += 1
    assert checked == 3 * len(cells.strategies)


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_host_statement_matches_every_range_file(case):
    cells = rc.case_cells(case)
    projection = rs.project_cells(cells)
    _, _, joint = rc.case_joint(case, cells)
    weights = rc.case_weights(case)
    S = len(cells.strategies)
    total = np.zeros((2, S), dtype=np.int64)
    for start, stop, member, maxima in rc.case_ranges(case):
        got = rs.host_root_bootstrap(projection.roots, projection.required_k, projection.wins, projection.exposures, weights, start, stop,
                                     case["top_n"], joint.observed, joint.expected, joint.observed_across, joint.expected_across,
                                     want_membership=True)
        assert got["membership"].shape == (stop - start, 2, S) and got["membership"].dtype == np.uint8
        assert got["membership"].tobytes() == member.tobytes()
        assert got["maxima"].shape == (stop - start,) and got["maxima"].tobytes() == maxima.tobytes()
        assert np.array_equal(got["top_counts"], member.sum(axis=0, dtype=np.int64))
        total += got["top_counts"]
    top_only = rs.host_root_bootstrap(projection.roots, projection.required_k, projection.wins, projection.exposures, weights, 0,
                                      case["replicates"], case["top_n"])
    assert top_only["maxima"] is None and top_only["membership"] is None and np.array_equal(top_only["top_counts"], total)
    if case["name"] == "k234":  # the zero-exposure cell: 12 of 13 batches of (11, 2) are eligible, all 13 of (23, 2)
        assert [len(w) for w in projection.wins] == [12, 9, 2, 13, 9, 2]


@pytest.mark.parametrize("case", REDUCIBLE, ids=lambda c: c["name"])
def test_three_frames_match_reference_for_any_split(case):
    cells = rc.case_cells(case)
    for range_size in (None, 50, 7):  # ranges split at 0 / 7 / 50: one call's results
        tables = rs.root_stability_tables(StubEngine(), cells, range_size=range_size, across_k=rc.case_across(case), **rc.case_kwargs(case))
        assert sorted(tables) == ["root_bootstrap_top_n_inclusion", "root_discrepancies", "root_joint_discrepancy"]
        for name, table in tables.items():
            assert table.num_rows == case[name]["rows"] > 0
            assert rc.encode(table) == rc.decode(case[name]), name
    assert tables["root_discrepancies"].schema.equals(rs.discrepancy_schema())
    assert tables["root_bootstrap_top_n_inclusion"].schema.equals(rs.top_n_inclusion_schema())
    assert tables["root_joint_discrepancy"].schema.equals(rs.joint_summary_schema())


def test_all_invalid_has_zero_maxima_and_no_reduction():
    case = rc.by_name("all_invalid")
    cells = rc.case_cells(case)
    with pytest.raises(ValueError, match="no discrepancy has a finite expected MCSE"):
        rs.root_stability_tables(StubEngine(), cells, across_k=rc.case_across(case), **rc.case_kwargs(case))


def _save_case(case, tmp_path):
    paths = []
    matrices = rc.case_matrices(case)
    for root in case["roots"]:
        for k in case["required_k"]:
            path = tmp_path / f"root_{root}" / f"{k}p" / "performance_batch_matrix.npy"
            matrices[(root, k)].save(path)
            paths.append(path)
    return paths


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_seams_write_the_reference_range_files(case, tmp_path):
    paths = _save_case(case, tmp_path)
    _, _, joint = rc.case_joint(case)
    weights = rc.case_weights(case)
    observed_by_k = tuple((k, tuple(joint.observed[i]), tuple(joint.expected[i])) for i, k in enumerate(case["required_k"]))
    S = len(case["strategies"])
    for start, stop, member, maxima in rc.case_ranges(case):
        top_path, joint_path = tmp_path / f"top_{start}.npy", tmp_path / f"joint_{start}.npy"
        rs.write_top_n_range(StubEngine(), paths, tuple(case["roots"]), tuple(case["required_k"]), tuple(case["strategies"]), tuple(weights),
                             case["top_n"], start, stop, top_path)
        rs.write_joint_discrepancy_range(StubEngine(), paths, tuple(case["roots"]), tuple(case["required_k"]), tuple(case["strategies"]),
                                         tuple(weights), observed_by_k, tuple(joint.observed_across), tuple(joint.expected_across), start, stop,
                                         joint_path)
        got_top, got_joint = np.load(top_path), np.load(joint_path)
        assert got_top.dtype == np.dtype("u1") and got_top.shape == (stop - start, 2, S) and got_top.tobytes() == member.tobytes()
        assert got_joint.dtype == np.dtype("<f8") and got_joint.shape == (stop - start,) and got_joint.tobytes() == maxima.tobytes()


def _tiny(wins_a, exposures_a, wins_b=None, exposures_b=None):
    wins_b = wins_a if wins_b is None else wins_b
    exposures_b = exposures_a if exposures_b is None else exposures_b
    return dict(roots=(1, 2), ks=[2], wins=[np.asarray(wins_a), np.asarray(wins_b)], exposures=[np.asarray(exposures_a), np.asarray(exposures_b)],
                weights=[1.0], replicate_begin=0, replicate_end=5, top_n=1)


def test_refusals_of_the_host_statement():
    # one eligible batch row and it is fine: every draw is that row
    fine = rs.host_root_bootstrap(**_tiny([[1, 2, 3]], [[4, 4, 4]]))
    assert fine["top_counts"].tolist() == [[0, 0, 5], [0, 0, 5]]
    # one batch row whose exposure is zero: every resampled total is zero
    with pytest.raises(ValueError, match="zero complete-support exposure"):
        rs.host_root_bootstrap(**_tiny([[1, 0, 3]], [[4, 0, 4]]))
    with pytest.raises(ValueError, match="negative count"):
        rs.host_root_bootstrap(**_tiny([[1, -1, 3]], [[4, 4, 4]]))
    with pytest.raises(ValueError, match="2\\*\\*63"):
        rs.host_root_bootstrap(**_tiny([[1, 2, 3]] * 4, [[4, 4, 2 ** 61]] * 4))
    with pytest.raises(ValueError, match="a < b"):
        rs.host_root_bootstrap(**{**_tiny([[1, 2, 3]], [[4, 4, 4]]), "roots": (2, 2)})
    with pytest.raises(ValueError, match="one S"):
        rs.host_root_bootstrap(**_tiny([[1, 2, 3]], [[4, 4, 4]], [[1, 2]], [[4, 4]]))
    with pytest.raises(ValueError, match="top_n"):
        rs.host_root_bootstrap(**{**_tiny([[1, 2, 3]], [[4, 4, 4]]), "top_n": 4})
    group = dict(observed=np.zeros((1, 3)), expected=np.ones((1, 3)), observed_across=np.zeros(3), expected_across=np.ones(3))
    for name in ("observed", "observed_across"):
        for bad in (np.nan, np.inf):
            broken = {k: v.copy() for k, v in group.items()}
            broken[name].reshape(-1)[1] = bad
            with pytest.raises(ValueError, match="observed is not finite"):
                rs.host_root_bootstrap(**_tiny([[1, 2, 3]], [[4, 4, 4]]), **broken)
    with pytest.raises(ValueError, match="group of four"):
        rs.host_root_bootstrap(**_tiny([[1, 2, 3]], [[4, 4, 4]]), observed=np.zeros((1, 3)))
    # expected may be NaN, zero or negative: the column is no estimand
    odd = dict(group, expected=np.asarray([[np.nan, 0.0, -1.0]]), expected_across=np.asarray([np.nan, -0.0, -np.inf]))
    assert rs.host_root_bootstrap(**_tiny([[1, 2, 3]], [[4, 4, 4]]), **odd)["maxima"].tobytes() == np.zeros(5).tobytes()


def test_refusals_of_the_cells(tmp_path):
    case = rc.by_name("k234")
    matrices = rc.case_matrices(case)
    roots, ks = case["roots"], case["required_k"]
    with pytest.raises(ValueError, match="exactly two roots"):
        rs.check_cells(matrices, [11], ks)
    with pytest.raises(ValueError, match="exactly two roots"):
        rs.check_cells(matrices, [11, 11], ks)
    with pytest.raises(ValueError, match="exactly two roots"):
        rs.check_cells(matrices, [11, 23, 31], ks)
    missing = {key: m for key, m in matrices.items() if key != (23, 3)}
    with pytest.raises(ValueError, match=r"missing=\[\(23, 3\)\]"):
        rs.check_cells(missing, roots, ks)
    wrong_root = dict(matrices)
    wrong_root[(23, 3)] = matrices[(11, 3)]
    with pytest.raises(ValueError, match=r"root support \[11\], expected \[23\]"):
        rs.check_cells(wrong_root, roots, ks)
    other = dict(matrices)
    m = matrices[(23, 4)]
    other[(23, 4)] = type(m)(m.root_seed, m.k, m.batch_ids, m.strategies + 1, m.wins, m.exposures, m.completed, m.safety)
    with pytest.raises(ValueError, match="strategy support differs"):
        rs.check_cells(other, roots, ks)
    with pytest.raises(ValueError, match="strategy support differs"):
        rs.check_cells(matrices, roots, ks, strategies=case["strategies"][:-1])
    paths = _save_case(case, tmp_path)
    with pytest.raises(ValueError, match="strategy support differs"):
        rs.write_top_n_range(StubEngine(), paths, roots, ks, [s + 1 for s in case["strategies"]], rc.case_weights(case), 3, 0, 2, tmp_path / "x.npy")
    with pytest.raises(ValueError, match="root support"):
        rs.write_top_n_range(StubEngine(), paths, (11, 24), ks, case["strategies"], rc.case_weights(case), 3, 0, 2, tmp_path / "x.npy")
    cells = rs.check_cells(matrices, roots, ks)
    kw = rc.case_kwargs(case)
    with pytest.raises(ValueError, match="practical_delta_by_k is required"):
        rs.root_stability_tables(StubEngine(), cells, **{**kw, "practical_delta_by_k": None})
    with pytest.raises(ValueError, match="delta_across_k is required"):
        rs.root_stability_tables(StubEngine(), cells, **{**kw, "delta_across_k": None})
    with pytest.raises(ValueError, match="declared k weights"):
        rs.root_stability_tables(StubEngine(), cells, **{**kw, "declared_k_weights": {2: 0.5, 3: 0.5}})
    # no eligible batch in a cell: a zero exposure in every batch row
    m = matrices[(11, 4)]
    exposures, completed, wins = m.exposures.copy(), m.completed.copy(), m.wins.copy()
    exposures[0, 0] = completed[0, 0] = wins[0, 0] = 0
    exposures[1, 5] = completed[1, 5] = wins[1, 5] = 0
    none_left = dict(matrices)
    none_left[(11, 4)] = type(m)(m.root_seed, m.k, m.batch_ids, m.strategies, wins, exposures, completed, np.zeros_like(m.safety))
    with pytest.raises(ValueError, match="no positive-exposure batch vectors"):
        rs.project_cells(rs.check_cells(none_left, roots, ks))
