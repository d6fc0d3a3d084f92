"""The host statement of the round-robin inference (``farkle_ii_amd.rr_inference``) against the literal restatement of the reference's
h2h_inference.py in tests/rr_inference_literal.py, pair by pair on the synthetic family of tests/rr_inference_cases.py; its frames;
the config fields."""
from __future__ import annotations

import math

import numpy as np
import pytest
from scipy.stats import norm

import rr_inference_cases as cases
import rr_inference_literal as lit
from farkle_ii_amd import rr_inference as ri


@pytest.fixture(scope="module")
def family():
    n, roots, target, cap = cases.synthetic_family()
    counts = ri.combine_counts(roots, [target] * len(roots), [cap] * len(roots))
    return n, counts


@pytest.fixture(scope="module", params=[None, cases.DELTA_EQUIVALENCE], ids=["equivalence_off", "equivalence_on"])
def result(request, family):
    n, counts = family
    return request.param, ri.infer(n, counts, delta_equivalence=request.param, **cases.PARAMS)


def test_counts_keep_the_orders_apart(family):
    n, counts = family
    _, roots, target, cap = cases.synthetic_family()
    assert counts.shape == (66, 2, 9) and counts.dtype == np.int64
    assert np.array_equal(counts[:, :, :5], roots[0].astype(np.int64) + roots[1])
    assert (counts[:, :, 5] == 2 * target).all() and (counts[:, :, 6] == 2 * cap).all() and (counts[:, :, 7] == 2).all()
    short = cases._pairs(n).index(cases.SHORT)
    assert counts[short, 0, 8] == 1 and counts[short, 1, 8] == 2 and (np.delete(counts[:, :, 8], short, axis=0) == 2).all()


def test_pairs_against_the_literal_restatement(result):
    equivalence, host = result
    rows = host["rows"]
    alpha, family_pairs = cases.PARAMS["family_alpha"], 66
    tested = (rows["flags"] & ri.FLAG_INFERENTIAL) != 0
    assert tested.sum() == 65 and not tested[cases._pairs(cases.N).index(cases.SHORT)]
    for r in rows[tested]:
        args = (int(r["seat1_a_wins_ab"]), int(r["n_ab"]), int(r["seat1_b_wins_ba"]), int(r["n_ba"]))
        difference, null_proportion, z, p = lit.score_test(*args)
        assert (r["raw_order_rate_difference"], r["score_null_proportion"], r["score_z"], r["score_p_value"]) == (difference, null_proportion, z, p)
        assert r["d_ab"] == 0.5 * difference and r["q_ab"] == args[0] / args[1] and r["q_ba"] == args[2] / args[3]
        assert math.isclose(r["balanced_a_win_rate"], 0.5 + r["d_ab"], rel_tol=0.0, abs_tol=1e-15)  # the alias check of :839-841
        for a, names in ((alpha, ("ordinary_d_low", "ordinary_d_high")), (alpha / family_pairs, ("simultaneous_d_low", "simultaneous_d_high"))):
            low, high = lit.interval(*args, a)
            assert abs(2.0 * r[names[0]] - low) <= lit.BOUND_TOL and abs(2.0 * r[names[1]] - high) <= lit.BOUND_TOL
    # Holm: bit-equal to the literal _holm_adjust over the working p-values
    adjusted, place = lit.holm(np.where(tested, rows["score_p_value"], 1.0))
    assert rows["holm_adjusted_p"][tested].tobytes() == adjusted[tested].tobytes() and np.isnan(rows["holm_adjusted_p"][~tested]).all()
    assert np.array_equal(rows["holm_order"], np.where(tested, place, 0))
    # the decision chain of :886-909, restated per pair
    for r in rows:
        eligible = bool(r["flags"] & ri.FLAG_ELIGIBLE)
        low, high = r["simultaneous_d_low"], r["simultaneous_d_high"]
        if not eligible:
            want = "unresolved_nonviable"
        elif low > 0.03:
            want = "practical_dominance_a"
        elif high < -0.03:
            want = "practical_dominance_b"
        elif r["flags"] & ri.FLAG_REJECT:
            want = "statistical_only_advantage_a" if r["d_ab"] > 0.0 else "statistical_only_advantage_b"
        elif equivalence is not None and low > -equivalence and high < equivalence:
            want = "equivalent"
        else:
            want = "unresolved"
        assert ri.DECISION_CLASSES[r["decision_class"]] == want
    cases.assert_margins(host, 0.03, equivalence, alpha)


def test_the_family_holds_every_case(result):
    equivalence, host = result
    rows = host["rows"]
    pairs = cases._pairs(cases.N)
    at = {pair: rows[pairs.index(pair)] for pair in pairs}
    ties = [at[p] for p in ((0, 1), (0, 2), (1, 2), (3, 4), (5, 6))]
    assert len({t["score_p_value"] for t in ties}) == 1 and [int(t["holm_order"]) for t in ties] == sorted(int(t["holm_order"]) for t in ties)
    zeros = [at[p] for p in ((0, 3), (1, 4), (2, 5))]
    assert all(t["score_p_value"] == 0.0 and abs(t["score_z"]) > 60 for t in zeros) and [int(t["holm_order"]) for t in zeros] == [1, 2, 3]
    for p in ((0, 4), (1, 5)):
        assert at[p]["score_z"] == 0.0 and at[p]["score_p_value"] == 1.0 and at[p]["simultaneous_d_low"] == -at[p]["simultaneous_d_high"]
    short = at[cases.SHORT]
    assert short["flags"] == ri.FLAG_OPERATIONAL and short["holm_order"] == 0 and np.isnan(short["score_z"]) and short["decision_class"] == 6
    st = host["strategies"]
    assert st[:, 11].tolist() == [0 if s in cases.SHORT else 1 for s in range(cases.N)]   # inferentially viable
    assert st[:, 10].tolist() == [0 if s == cases.WEAK else 1 for s in range(cases.N)]    # operationally viable
    assert all(not (at[(s, cases.WEAK)]["flags"] & ri.FLAG_ELIGIBLE) and at[(s, cases.WEAK)]["decision_class"] == 6 for s in range(cases.WEAK))
    counts = host["class_counts"]
    assert counts.sum() == 66 and counts[6] == 12 and (counts[:4] > 0).all() and counts[5] > 0 and (counts[4] > 0) == (equivalence is not None)
    assert (st[:, :7].sum(axis=1) == 11).all() and st[:, 0].sum() == st[:, 1].sum() == counts[0] + counts[1]
    assert st[:, 2].sum() == st[:, 3].sum() == counts[2] + counts[3]


def test_rows_slice_and_pair_range(family):
    n, counts = family
    full = ri.infer(n, counts, **cases.PARAMS)
    part = ri.infer(n, counts, rows=(10, 25), **cases.PARAMS)
    assert part["rows"].tobytes() == full["rows"][10:25].tobytes() and np.array_equal(part["class_counts"], full["class_counts"])
    sub = ri.infer(n, counts[20:50], pair_begin=20, family_pair_count=66, **cases.PARAMS)  # a range of its own: Holm over 30 pairs
    assert sub["rows"]["pair_id"].tolist() == list(range(20, 50)) and sub["class_counts"].sum() == 30
    assert np.array_equal(sub["rows"]["simultaneous_d_low"], full["rows"]["simultaneous_d_low"][20:50], equal_nan=True)


def test_vectorised_intervals_against_the_plain_loop(family):
    """``intervals="bisection"`` (large families) finds a root of the same objective in the same bracket: within brentq's stated
    xtol + rtol |x| <= 1.01e-12 of the loop's, on the raw difference; everything that is not an interval bound is identical."""
    n, counts = family
    loop = ri.infer(n, counts, delta_equivalence=cases.DELTA_EQUIVALENCE, **cases.PARAMS)
    fast = ri.infer(n, counts, delta_equivalence=cases.DELTA_EQUIVALENCE, intervals="bisection", **cases.PARAMS)
    for name in cases.BOUND_FIELDS:
        assert np.nanmax(np.abs(2.0 * loop["rows"][name] - 2.0 * fast["rows"][name])) <= 1.01e-12
        assert np.array_equal(np.isnan(loop["rows"][name]), np.isnan(fast["rows"][name]))
    for name in cases.EXACT_FIELDS + ("score_p_value", "holm_adjusted_p", "holm_order"):
        assert loop["rows"][name].tobytes() == fast["rows"][name].tobytes(), name
    assert np.array_equal(loop["strategies"], fast["strategies"])


def test_host_statement_refuses_what_the_entry_refuses(family):
    n, counts = family
    for bad, match in ((dict(family_alpha=0.0), "family_alpha"), (dict(family_alpha=1.0), "family_alpha"), (dict(practical_delta=0.0), "practical_delta"),
                       (dict(delta_equivalence=1.0), "delta_equivalence"), (dict(min_candidate_completion_rate=1.5), "completion_rate"),
                       (dict(family_pair_count=65), "family_pair_count")):
        with pytest.raises(ValueError, match=match):
            ri.infer(n, counts, **{**cases.PARAMS, **bad})


def test_frames(family):
    n, counts = family
    ids = np.arange(100, 100 + n)
    host = ri.infer(n, counts, delta_equivalence=cases.DELTA_EQUIVALENCE, **cases.PARAMS)
    pairs = ri.pairs_frame(host["rows"], ids, delta_equivalence=cases.DELTA_EQUIVALENCE, **cases.PARAMS)
    assert len(pairs) == 66 and pairs["strategy_a"].iloc[0] == 100 and pairs["strategy_b"].iloc[-1] == 111
    short = cases._pairs(n).index(cases.SHORT)
    row = pairs.iloc[short]
    assert row["completion_status"] == "unresolved_nonviable" and row["n_ab"] is not None and str(row["n_ab"]) == "<NA>"
    assert str(row["holm_order"]) == "<NA>" and np.isnan(row["score_z"]) and row["no_test_p_value_convention"] == "null_reported_treated_as_one_for_holm"
    assert row["descriptive_completed_games"] == 4 * cases.TARGET - 1 and row["decision_class"] == "unresolved_nonviable"
    assert pairs["bonferroni_alpha_per_pair"].iloc[0] == 0.02 / 66 and bool(pairs["equivalence_enabled"].iloc[0])
    assert set(pairs["decision_class"]) == set(ri.DECISION_CLASSES)
    strategies = ri.strategies_frame(host["strategies"], ids)
    status = dict(zip(strategies["strategy"], strategies["candidate_status"]))
    assert status[100 + cases.WEAK] == "operationally_nonviable" and status[108] == status[109] == "inferentially_nonviable" and status[100] == "viable"
    weak = strategies.iloc[cases.WEAK]
    assert weak["completion_rate"] == weak["games_completed"] / weak["games_attempted"] < 0.99


def test_critical_values_and_config_defaults():
    assert ri.critical_values(0.02, 66) == (float(norm.isf(0.01)), float(norm.isf(0.02 / 66 / 2.0)))
    from farkle_ii_amd.config import AppConfig

    h = AppConfig().head2head
    assert (h.family_alpha, h.practical_delta, h.delta_equivalence, h.min_candidate_completion_rate) == (0.02, 0.03, None, 0.99)
