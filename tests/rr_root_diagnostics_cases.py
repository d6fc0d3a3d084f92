"""The families the per-root diagnostics tests run on, the facts about them that make them worth running, and the comparison of a
device result with the host statement.

``synthetic``: ``rr_inference_cases.synthetic_family()`` (12 strategies, 66 pairs, two roots) with the roots added as seeds (12, 11),
so that ``root_a`` is the root played second.  ``wide``: ``random_family(seed=7)`` with ``random_family(seed=8)`` as a second root
(300 strategies, 44 850 pairs: several sort and scan tiles)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import rr_inference_cases as cases
import rr_inference_literal as lit
from farkle_ii_amd import rr_root_diagnostics as rd

PARAMS = cases.PARAMS
SYNTHETIC_SEEDS = (12, 11)  # in arrival order: root_a is 11, the second root of the family
WIDE_SEEDS = (7, 8)


def assert_margins(host: dict, family_alpha: float) -> None:
    """No decision hangs on the last digits: no adjusted p of any root within a factor 1 +- 1e-9 of alpha (``rr_inference_cases.
    assert_margins``; the diagnostics read no interval bound)."""
    for rows in host["rows"]:
        adjusted = rows["holm_adjusted_p"][(rows["flags"] & 1) != 0]
        assert (np.abs(adjusted / family_alpha - 1.0) > 1e-9).all()


def alpha_margin(host: dict, family_alpha: float) -> float:
    return min(float(np.abs(rows["holm_adjusted_p"][(rows["flags"] & 1) != 0] / family_alpha - 1.0).min()) for rows in host["rows"])


@lru_cache(maxsize=None)
def synthetic() -> dict:
    n, roots, target, cap = cases.synthetic_family()
    host = rd.diagnose(n, roots, SYNTHETIC_SEEDS, [target] * 2, [cap] * 2, **PARAMS)
    assert_synthetic_facts(host)
    return {"n": n, "roots": roots, "seeds": SYNTHETIC_SEEDS, "target": target, "cap": cap, "host": host}


def assert_synthetic_facts(host: dict) -> None:
    """What the synthetic family holds for the diagnostics (rows[0] is seed 11 = the family's root 1, rows[1] seed 12 = root 0)."""
    rows, agreement = host["rows"], host["agreement"]
    assert host["roots"].tolist() == [11, 12] and rows.shape == (2, 66)
    assert (rows[0]["diagnostic_decision"] != rows[1]["diagnostic_decision"]).sum() == 4
    available = (agreement["flags"] & rd.AGREE_AVAILABLE) != 0
    assert available.sum() == 65 and (available & ((agreement["flags"] & rd.AGREE_DIRECTION) == 0)).sum() == 4
    for r, weak_rejections in ((0, 4), (1, 5)):
        assert (rows[r]["d_ab"] == 0.0).sum() == 2
        flags = rows[r]["flags"]
        assert (((flags & 8) != 0) & ((flags & 4) == 0)).sum() == weak_rejections  # rejected before viability, not claim-eligible (WEAK)
    short = cases._pairs(cases.N).index(cases.SHORT)  # short in root 1 only: no test in root 0 either
    for r in range(2):
        assert rows[r][short]["flags"] == 2 and rows[r][short]["holm_order"] == 0 and np.isnan(rows[r][short]["d_ab"])
    assert not available[short]
    assert alpha_margin(host, PARAMS["family_alpha"]) >= 0.2
    assert_margins(host, PARAMS["family_alpha"])


@lru_cache(maxsize=None)
def wide() -> dict:
    n, first, target, cap = cases.random_family(seed=7)
    _, second, _, _ = cases.random_family(seed=8)
    roots = [first[0], second[0]]
    host = rd.diagnose(n, roots, WIDE_SEEDS, [target] * 2, [cap] * 2, intervals="bisection", **PARAMS)
    assert host["summary"][0] == 44_850 and host["summary"][1] == 44_836
    assert 0.03 <= alpha_margin(host, PARAMS["family_alpha"]) < 0.031
    assert_margins(host, PARAMS["family_alpha"])
    return {"n": n, "roots": roots, "seeds": WIDE_SEEDS, "target": target, "cap": cap, "host": host}


ROOT_EXACT_FIELDS = ("pair_id", "strategy_a", "strategy_b", "games_attempted", "games_completed", "games_safety_limit", "n_ab", "n_ba",
                     "seat1_a_wins_ab", "seat1_b_wins_ba", "flags", "diagnostic_decision", "completion_game_rate", "q_ab", "q_ba", "d_ab",
                     "score_null_proportion", "score_z")
ROOT_BOUND_FIELDS = ("ordinary_d_low", "ordinary_d_high")


def compare(dev: dict, host: dict) -> None:
    """A device result against the host statement of the same states and parameters, by the rules of ``rr_inference_cases.compare``."""
    from scipy.stats import norm

    assert dev["roots"].dtype == np.uint64 and dev["roots"].tolist() == host["roots"].tolist()
    assert dev["rows"].shape == host["rows"].shape
    for got, want in zip(dev["rows"], host["rows"]):
        for name in ROOT_EXACT_FIELDS:  # bit-equal (NaN where a pair has no test, in both)
            assert got[name].tobytes() == want[name].tobytes(), name
        assert not got["pad"].any()
        tested = (want["flags"] & 1) != 0
        for name in ROOT_BOUND_FIELDS + ("score_p_value", "holm_adjusted_p"):
            assert np.array_equal(np.isnan(got[name]), ~tested), name
        for name in ROOT_BOUND_FIELDS:  # the halved bounds: half of 2.5e-12
            assert np.abs(got[name][tested] - want[name][tested]).max(initial=0.0) <= 0.5 * lit.BOUND_TOL, name
        z = np.abs(want["score_z"][tested])
        p_ref, p_dev = 2.0 * norm.sf(z), got["score_p_value"][tested]
        normal = p_ref >= 2.3e-308
        assert (np.abs(p_dev[normal] - p_ref[normal]) <= cases.p_value_bound(z[normal]) * p_ref[normal]).all()
        assert (p_dev[z >= 39.0] == 0.0).all()
        # Holm is exact as a function of the device's own p
        adjusted, place = lit.holm(np.where(tested, got["score_p_value"], 1.0))
        assert got["holm_adjusted_p"][tested].tobytes() == adjusted[tested].tobytes()
        assert np.array_equal(got["holm_order"], np.where(tested, place, 0))
    assert dev["agreement"].tobytes() == host["agreement"].tobytes()
    assert np.array_equal(dev["summary"], host["summary"])
    assert np.float64(dev["max_abs_discrepancy"]).tobytes() == np.float64(host["max_abs_discrepancy"]).tobytes()
