"""Round-robin inference: the score test, the score intervals, Holm's adjustment and the decision class of every pair.

``Engine.rr_inference`` (``fk_rr_inference``) runs the reference's ``src/farkle/analysis/h2h_inference.py`` over pair counts that
stay on the device (``Engine.h2h_round_robin_resident`` / ``Engine.rr_counts_add``).  This module is the host side:

* ``combine_counts`` — the accumulator of the device, from block states (``_combine_within_order``, :563-635);
* ``score_test`` / ``statistic_at_difference`` / ``score_interval`` / ``holm_adjust`` — the host statement of the statistics
  (:68-99, :142-188, :191-277, :280-295): NumPy where that is easy, a plain loop with ``scipy.optimize.brentq`` for the intervals;
* ``infer`` — the host statement of the whole entry (``_viability_status`` :638-700, ``_pairwise_estimates`` :703-915), returning what
  ``Engine.rr_inference`` returns; the tests compare the two;
* ``pairs_frame`` / ``strategies_frame`` — the tables ``farkle round-robin --inference`` writes, columns named as in
  ``_pairwise_estimates`` for what is computed.

The interval is the reference's own complete inversion of the uncorrected constrained score statistic
(``_score_difference_interval_fallback``); the library route of the interval (``confint_proportions_2indep``) is not reproduced.

Left out of the frames (the reference computes them from its schedule hashes and block manifests, which this package does not have):
``family_hash``, ``replacement_attempt_count`` and its per-strategy sums, ``score_test_id``, ``interval_method_id``,
``h2h_method_version``.  The three columns the reference derives from its power plan —
``planned_target_power_conditional_on_completed_support``, ``planned_worst_scenario_power_conditional_on_completed_support``,
``power_support_status`` — are added by ``with_plan_columns`` when the run planned its own block size (``farkle round-robin
--plan-power``, ``farkle_ii_amd/h2h_power.py``); a run that was handed its block size has no plan to quote.  Also out of scope: sidecars and
completion stamps, several ranks, resuming.  The graphs the reference's ``dominance.py`` builds from these classes are
``Engine.rr_dominance`` and ``farkle_ii_amd/dominance.py``; its ``_root_specific_diagnostics`` (the inference per root and the
cross-root agreement) is ``Engine.rr_root_diagnostics`` and ``farkle_ii_amd/rr_root_diagnostics.py``.
"""
from __future__ import annotations

import math
from typing import Any, Sequence

import numpy as np

from .backend import RR_CLASSES, RR_PAIR_ROW_DTYPE, RR_STRATEGY_COLS
from .round_robin import pair_count, pair_ids

COUNT_COLS = ("games_attempted", "games_completed", "games_safety_limit", "wins_seat1", "wins_seat2", "n_completed_required",
              "max_attempts", "root_order_cell_count", "resolved_root_order_cell_count")  # the accumulator's columns per (pair, order)
DECISION_CLASSES = ("practical_dominance_a", "practical_dominance_b", "statistical_only_advantage_a", "statistical_only_advantage_b",
                    "equivalent", "unresolved", "unresolved_nonviable")  # FK_RR_PRACTICAL_DOMINANCE_A ..
STRATEGY_CLASS_COLS = ("practical_dominance_wins", "practical_dominance_losses", "statistical_only_advantage_wins",
                       "statistical_only_advantage_losses", "equivalent", "unresolved", "unresolved_nonviable", "games_attempted",
                       "games_completed", "games_safety_limit", "operationally_viable", "inferentially_viable")  # FK_RR_STRATEGY_COLS
FLAG_INFERENTIAL, FLAG_OPERATIONAL, FLAG_ELIGIBLE, FLAG_REJECT_BEFORE, FLAG_REJECT = 1, 2, 4, 8, 16  # FK_RR_FLAG_*
DEFAULT_ROWS_LIMIT = 1 << 22  # `farkle round-robin --inference` writes every pair of a range up to this size unless --rows says otherwise


def combine_counts(states: Sequence[Any], targets: Sequence[int], max_attempts: Sequence[int]) -> np.ndarray:
    """Block states of several roots, each ``[pairs, 2, 5]`` with its target and attempt cap -> int64 ``[pairs, 2, 9]`` (``COUNT_COLS``)."""
    out = None
    for st, target, cap in zip(states, targets, max_attempts, strict=True):
        st = np.asarray(st).astype(np.int64)
        if st.ndim != 3 or st.shape[1:] != (2, 5):
            raise ValueError(f"states must have shape (pairs, 2, 5), got {st.shape}")
        if out is None:
            out = np.zeros((st.shape[0], 2, len(COUNT_COLS)), dtype=np.int64)
        if st.shape[0] != out.shape[0]:
            raise ValueError("every root must cover the same pair range")
        out[:, :, :5] += st
        out[:, :, 5] += int(target)
        out[:, :, 6] += int(cap)
        out[:, :, 7] += 1
        out[:, :, 8] += st[:, :, 1] == int(target)
    if out is None:
        raise ValueError("no states to combine")
    return out


def score_test(count1, nobs1, count2, nobs2) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``two_proportion_score_test`` over arrays: ``(difference, null_proportion, statistic, p_value)``."""
    from scipy.stats import norm

    c1, n1, c2, n2 = (np.asarray(v, dtype=np.int64) for v in (count1, nobs1, count2, nobs2))
    if (n1 <= 0).any() or (n2 <= 0).any() or (c1 < 0).any() or (c2 < 0).any() or (c1 > n1).any() or (c2 > n2).any():
        raise ValueError("score tests need positive sample sizes and counts within them")
    difference = c1 / n1 - c2 / n2
    null_proportion = (c1 + c2) / (n1 + n2)
    variance = null_proportion * (1.0 - null_proportion) * (1.0 / n1 + 1.0 / n2)
    positive = variance > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        statistic = np.where(positive, difference / np.sqrt(np.where(positive, variance, 1.0)),
                             np.where(difference == 0.0, 0.0, np.copysign(np.inf, difference)))
    p_value = np.where(positive, 2.0 * norm.sf(np.abs(statistic)), np.where(difference == 0.0, 1.0, 0.0))
    return difference, null_proportion, statistic, p_value


def statistic_at_difference(count1: int, nobs1: int, count2: int, nobs2: int, difference: float) -> float:
    """``_score_statistic_at_difference``: the uncorrected constrained score statistic of H0 ``p1 - p2 = difference``."""
    c1, n1, c2, n2, d = int(count1), int(nobs1), int(count2), int(nobs2), float(difference)
    if d <= -1.0:
        p1, p2 = 0.0, 1.0
    elif d >= 1.0:
        p1, p2 = 1.0, 0.0
    elif d == 0.0:
        p1 = p2 = (c1 + c2) / (n1 + n2)
    else:  # the constrained maximum-likelihood rates: the trigonometric root of a cubic
        big_n, hits = n1 + n2, c1 + c2
        k2 = (n1 + 2 * n2) * d - big_n - hits
        k1 = (c2 * d - big_n - 2 * c2) * d + hits
        k0 = c2 * d * (1.0 - d)
        q = (k2 / (3 * big_n)) ** 3 - k1 * k2 / (6 * big_n**2) + k0 / (2 * big_n)
        under = (k2 / (3 * big_n)) ** 2 - k1 / (3 * big_n)
        root = math.copysign(math.sqrt(max(0.0, under)), q) if q != 0.0 else 0.0
        if root == 0.0:
            p2 = -k2 / (3 * big_n)
        else:
            angle = (math.pi + math.acos(max(-1.0, min(1.0, q / root**3)))) / 3.0
            p2 = 2.0 * root * math.cos(angle) - k2 / (3 * big_n)
        p1 = max(0.0, min(1.0, p2 + d))
        p2 = max(0.0, min(1.0, p2))
    variance = p1 * (1.0 - p1) / n1 + p2 * (1.0 - p2) / n2
    gap = (c1 / n1 - c2 / n2) - d
    if variance > 0.0:
        return gap / math.sqrt(variance)
    return 0.0 if gap == 0.0 else math.copysign(math.inf, gap)


def _bound(c1: int, n1: int, c2: int, n2: int, observed: float, endpoint: float, critical_value: float) -> float:
    from scipy.optimize import brentq

    if observed == endpoint:
        return endpoint

    def excess(d: float) -> float:
        s = statistic_at_difference(c1, n1, c2, n2, d)
        return 1.0 if math.isinf(s) else abs(s) - critical_value

    inner, span = observed, endpoint - observed
    for e in range(52, -1, -1):
        outer = observed + span * 2.0**-e
        if outer == inner:
            continue
        if excess(outer) >= 0.0:
            return float(brentq(excess, min(inner, outer), max(inner, outer), xtol=1e-12, rtol=1e-14))
        inner = outer
    raise RuntimeError("no bracket for a score interval bound")


def score_interval(count1: int, nobs1: int, count2: int, nobs2: int, critical_value: float) -> tuple[float, float]:
    """``_score_difference_interval_fallback`` at ``critical_value = norm.isf(alpha / 2)``: ``(low, high)`` of the raw difference."""
    c1, n1, c2, n2 = int(count1), int(nobs1), int(count2), int(nobs2)
    observed = c1 / n1 - c2 / n2
    if observed > 0.0:
        low, high = score_interval(c2, n2, c1, n1, critical_value)
        return -high, -low
    low = _bound(c1, n1, c2, n2, observed, -1.0, critical_value)
    high = _bound(c1, n1, c2, n2, observed, 1.0, critical_value)
    if c1 == c2 and n1 == n2:
        widest = max(abs(low), abs(high))
        return -widest, widest
    return low, high


def statistic_at_difference_many(c1, n1, c2, n2, d) -> np.ndarray:
    """``statistic_at_difference`` over float64 arrays (counts below 2^53 are exact in them), the same operations in the same order
    with the powers written as products, as the device header writes them."""
    with np.errstate(divide="ignore", invalid="ignore"):
        big_n, hits = n1 + n2, c1 + c2
        k2 = (n1 + 2.0 * n2) * d - big_n - hits
        k1 = (c2 * d - big_n - 2.0 * c2) * d + hits
        k0 = c2 * d * (1.0 - d)
        shift = k2 / (3.0 * big_n)
        q = shift * shift * shift - k1 * k2 / (6.0 * big_n * big_n) + k0 / (2.0 * big_n)
        under = shift * shift - k1 / (3.0 * big_n)
        root = np.where(q != 0.0, np.copysign(np.sqrt(np.maximum(0.0, under)), q), 0.0)
        flat = root == 0.0
        cosine = np.clip(q / np.where(flat, 1.0, root * root * root), -1.0, 1.0)
        p2 = np.where(flat, -k2 / (3.0 * big_n), 2.0 * root * np.cos((math.pi + np.arccos(cosine)) / 3.0) - shift)
        p1 = np.clip(p2 + d, 0.0, 1.0)
        p2 = np.clip(p2, 0.0, 1.0)
        pooled = hits / big_n
        p1 = np.where(d <= -1.0, 0.0, np.where(d >= 1.0, 1.0, np.where(d == 0.0, pooled, p1)))
        p2 = np.where(d <= -1.0, 1.0, np.where(d >= 1.0, 0.0, np.where(d == 0.0, pooled, p2)))
        variance = p1 * (1.0 - p1) / n1 + p2 * (1.0 - p2) / n2
        gap = (c1 / n1 - c2 / n2) - d
        return np.where(variance > 0.0, gap / np.sqrt(np.where(variance > 0.0, variance, 1.0)),
                        np.where(gap == 0.0, 0.0, np.copysign(np.inf, gap)))


def score_interval_many(count1, nobs1, count2, nobs2, critical_value: float) -> tuple[np.ndarray, np.ndarray]:
    """``score_interval`` over arrays, for families too large for the plain loop: the same swap, bracket and symmetric rule; inside the
    bracket, bisection to the last bit instead of ``brentq`` (a root of the same objective in the same bracket: within ``brentq``'s
    ``xtol`` of what the loop returns, which tests/test_rr_inference_cpu.py checks)."""
    c1, n1, c2, n2 = (np.asarray(v, dtype=np.float64).copy() for v in (count1, nobs1, count2, nobs2))
    swapped = c1 / n1 - c2 / n2 > 0.0
    c1[swapped], c2[swapped] = c2[swapped], c1[swapped].copy()
    n1[swapped], n2[swapped] = n2[swapped], n1[swapped].copy()
    observed = c1 / n1 - c2 / n2

    def rejects(d):
        s = statistic_at_difference_many(c1, n1, c2, n2, d)
        return np.where(np.isinf(s), 1.0, np.abs(s) - critical_value) >= 0.0

    bounds = []
    for endpoint in (-1.0, 1.0):
        accepted, rejected = observed.copy(), np.full_like(observed, endpoint)
        open_ = observed != endpoint  # no bracket yet
        span = endpoint - observed
        for e in range(52, -1, -1):
            trial = observed + span * 2.0**-e
            hit = open_ & (trial != accepted) & rejects(trial)
            rejected = np.where(hit, trial, rejected)
            accepted = np.where(open_ & ~hit, trial, accepted)
            open_ &= ~hit
        if open_.any():
            raise RuntimeError("no bracket for a score interval bound")
        live = observed != endpoint
        for _ in range(64):
            mid = 0.5 * (accepted + rejected)
            inside = live & (mid != accepted) & (mid != rejected)
            if not inside.any():
                break
            out = rejects(mid)
            rejected = np.where(inside & out, mid, rejected)
            accepted = np.where(inside & ~out, mid, accepted)
        bounds.append(np.where(live, 0.5 * (accepted + rejected), endpoint))
    low, high = bounds
    same = (c1 == c2) & (n1 == n2)
    widest = np.maximum(np.abs(low), np.abs(high))
    low, high = np.where(same, -widest, low), np.where(same, widest, high)
    return np.where(swapped, -high, low), np.where(swapped, -low, high)


def holm_adjust(p_values) -> tuple[np.ndarray, np.ndarray]:
    """``_holm_adjust``: ``(adjusted, positions)``, positions 1-based in the stable ascending order."""
    p = np.asarray(p_values, dtype=np.float64)
    count = len(p)
    order = np.argsort(p, kind="stable")
    running = np.maximum.accumulate((count - np.arange(count)).astype(np.float64) * p[order]) if count else np.zeros(0)
    adjusted = np.empty(count, dtype=np.float64)
    adjusted[order] = np.minimum(1.0, running)
    positions = np.empty(count, dtype=np.int64)
    positions[order] = np.arange(1, count + 1, dtype=np.int64)
    return adjusted, positions


def critical_values(family_alpha: float, family_pair_count: int) -> tuple[float, float]:
    """``norm.isf(alpha / 2)`` of the ordinary and of the Bonferroni alpha (``family_alpha / family_pair_count``)."""
    from scipy.stats import norm

    return float(norm.isf(family_alpha / 2.0)), float(norm.isf(family_alpha / family_pair_count / 2.0))


def check_params(n_pairs: int, family_alpha: float, practical_delta: float, delta_equivalence: float | None,
                 min_candidate_completion_rate: float, family_pair_count: int) -> None:
    """What ``fk_rr_inference`` refuses, with the same conditions."""
    if not 0.0 < family_alpha < 1.0:
        raise ValueError(f"family_alpha must be in (0, 1), got {family_alpha}")
    if not practical_delta > 0.0:
        raise ValueError(f"practical_delta must be positive, got {practical_delta}")
    if delta_equivalence is not None and not 0.0 < delta_equivalence < 1.0:
        raise ValueError(f"delta_equivalence must be in (0, 1) or None, got {delta_equivalence}")
    if not 0.0 <= min_candidate_completion_rate <= 1.0:
        raise ValueError(f"min_candidate_completion_rate must be in [0, 1], got {min_candidate_completion_rate}")
    if family_pair_count < n_pairs:
        raise ValueError(f"family_pair_count {family_pair_count} is smaller than the {n_pairs} pairs of the range")


def viability(n: int, counts: np.ndarray, pair_begin: int, min_candidate_completion_rate: float) -> dict:
    """``_viability_status`` (:638-700) over ``counts`` (``combine_counts``): the pairs' ids and ``viable`` bits, the per-strategy
    incident sums ``[n, 4]`` (attempted, completed, safety, nonviable pairs) and the strategies' two flags."""
    pid, i, j = pair_ids(n, pair_begin, pair_begin + counts.shape[0])
    ab, ba = counts[:, 0], counts[:, 1]
    viable = ((ab[:, 7] > 0) & (ab[:, 8] == ab[:, 7]) & (ab[:, 1] == ab[:, 5]) & (ba[:, 7] > 0) & (ba[:, 8] == ba[:, 7]) & (ba[:, 1] == ba[:, 5])
              & (ab[:, 1] == ba[:, 1]))
    # incident sums, one division, "all incident pairs viable"
    sums = np.zeros((n, 4), dtype=np.int64)
    for idx in (i, j):
        for c, values in enumerate((ab[:, 0] + ba[:, 0], ab[:, 1] + ba[:, 1], ab[:, 2] + ba[:, 2], (~viable).astype(np.int64))):
            np.add.at(sums[:, c], idx, values)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = sums[:, 1] / sums[:, 0]
    operational = (sums[:, 0] > 0) & (rate >= float(min_candidate_completion_rate))
    return {"pair_id": pid, "i": i, "j": j, "viable": viable, "sums": sums, "operational": operational, "inferential": sums[:, 3] == 0}


def infer(n: int, counts, pair_begin: int = 0, family_alpha: float = 0.02, practical_delta: float = 0.03,
          delta_equivalence: float | None = None, min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None,
          rows: tuple[int, int] | None = None, intervals: str = "brentq") -> dict:
    """The host statement of ``fk_rr_inference`` over ``counts`` (``combine_counts``) of pairs ``[pair_begin, pair_begin + len(counts))``
    of an ``n``-row table: ``{"class_counts", "strategies", "rows"}`` as ``Engine.rr_inference`` returns them (``rows``: every pair of
    the range unless a pair-id range is given).  ``intervals``: ``"brentq"`` is the plain loop over ``score_interval``, ``"bisection"``
    the vectorised ``score_interval_many`` for families too large for the loop."""
    if intervals not in ("brentq", "bisection"):
        raise ValueError(f"intervals must be 'brentq' or 'bisection', got {intervals!r}")
    counts = np.asarray(counts, dtype=np.int64)
    n, begin = int(n), int(pair_begin)
    n_pairs = counts.shape[0]
    family = pair_count(n) if family_pair_count is None else int(family_pair_count)
    check_params(n_pairs, family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family)
    status = viability(n, counts, begin, min_candidate_completion_rate)
    pid, i, j, viable, sums, operational, inferential = (status[k] for k in ("pair_id", "i", "j", "viable", "sums", "operational", "inferential"))
    ab, ba = counts[:, 0], counts[:, 1]
    pair_operational = operational[i] & operational[j]
    eligible = viable & pair_operational

    out = np.zeros(n_pairs, dtype=RR_PAIR_ROW_DTYPE)
    out["pair_id"], out["strategy_a"], out["strategy_b"] = pid, i, j
    for c, name in enumerate(("games_attempted", "games_completed", "games_safety_limit")):
        out[name] = ab[:, c] + ba[:, c]
    out["n_completed_required"] = ab[:, 5] + ba[:, 5]
    n_ab, n_ba, x_ab, x_ba, a_wins_ba = ab[:, 1], ba[:, 1], ab[:, 3], ba[:, 3], ba[:, 4]
    out["n_ab"], out["n_ba"], out["seat1_a_wins_ab"], out["seat1_b_wins_ba"], out["seat2_a_wins_ba"] = n_ab, n_ba, x_ab, x_ba, a_wins_ba
    out["balanced_a_wins"] = x_ab + a_wins_ba
    with np.errstate(divide="ignore", invalid="ignore"):
        out["completion_game_rate"] = out["games_completed"] / out["games_attempted"]
    doubles = ("q_ab", "q_ba", "raw_order_rate_difference", "d_ab", "score_null_proportion", "score_z", "score_p_value", "ordinary_d_low",
               "ordinary_d_high", "simultaneous_d_low", "simultaneous_d_high", "balanced_a_win_rate", "holm_adjusted_p")
    for name in doubles:
        out[name] = np.nan
    v = np.flatnonzero(viable)
    crit_ordinary, crit_simultaneous = critical_values(family_alpha, family)
    if len(v):
        difference, null_proportion, z, p = score_test(x_ab[v], n_ab[v], x_ba[v], n_ba[v])
        out["q_ab"][v], out["q_ba"][v] = x_ab[v] / n_ab[v], x_ba[v] / n_ba[v]
        out["raw_order_rate_difference"][v], out["d_ab"][v] = difference, 0.5 * difference
        out["score_null_proportion"][v], out["score_z"][v], out["score_p_value"][v] = null_proportion, z, p
        out["balanced_a_win_rate"][v] = (x_ab[v] + a_wins_ba[v]) / (n_ab[v] + n_ba[v])
        wanted = v if rows is None else v[(pid[v] >= int(rows[0])) & (pid[v] < int(rows[1]))]
        for idx, crit, names in ((v, crit_simultaneous, ("simultaneous_d_low", "simultaneous_d_high")),
                                 (wanted, crit_ordinary, ("ordinary_d_low", "ordinary_d_high"))):
            if intervals == "bisection":
                low, high = score_interval_many(x_ab[idx], n_ab[idx], x_ba[idx], n_ba[idx], crit)
            else:  # the plain loop
                both = [score_interval(int(x_ab[q]), int(n_ab[q]), int(x_ba[q]), int(n_ba[q]), crit) for q in idx]
                low, high = (np.array([b[k] for b in both], dtype=np.float64) for k in (0, 1))
            out[names[0]][idx], out[names[1]][idx] = 0.5 * low, 0.5 * high  # :851-854
    adjusted, positions = holm_adjust(np.where(viable, np.nan_to_num(out["score_p_value"], nan=1.0), 1.0))
    out["holm_order"] = np.where(viable, positions, 0)
    out["holm_adjusted_p"] = np.where(viable, adjusted, np.nan)
    reject_before = viable & (adjusted <= float(family_alpha))
    reject = reject_before & eligible
    out["flags"] = (viable * FLAG_INFERENTIAL + pair_operational * FLAG_OPERATIONAL + eligible * FLAG_ELIGIBLE + reject_before * FLAG_REJECT_BEFORE
                    + reject * FLAG_REJECT).astype(np.uint8)
    low, high, effect = out["simultaneous_d_low"], out["simultaneous_d_high"], out["d_ab"]
    with np.errstate(invalid="ignore"):
        equivalent = np.zeros(n_pairs, dtype=bool) if delta_equivalence is None else (low > -delta_equivalence) & (high < delta_equivalence)
        cls = np.select([~eligible, low > practical_delta, high < -practical_delta, reject & (effect > 0.0), reject, equivalent],
                        [6, 0, 1, 2, 3, 4], default=5)
    out["decision_class"] = cls.astype(np.uint8)
    class_counts = np.bincount(cls, minlength=RR_CLASSES).astype(np.int64)
    strategies = np.zeros((n, RR_STRATEGY_COLS), dtype=np.int64)
    np.add.at(strategies, (i, cls), 1)
    np.add.at(strategies, (j, np.where(cls < 4, cls ^ 1, cls)), 1)  # B's side of the pair: a win of A is a loss of B
    strategies[:, 7:10] = sums[:, :3]
    strategies[:, 10], strategies[:, 11] = operational, inferential
    if rows is not None:
        out = out[(pid >= int(rows[0])) & (pid < int(rows[1]))]
    return {"class_counts": class_counts, "strategies": strategies, "rows": out}


def _ids(strategy_ids, n: int) -> np.ndarray:
    ids = np.arange(n, dtype=np.int64) if strategy_ids is None else np.asarray(strategy_ids, dtype=np.int64)
    if ids.shape != (n,):
        raise ValueError(f"strategy_ids must name the {n} rows of the table")
    return ids


def pairs_frame(rows: np.ndarray, strategy_ids=None, n: int | None = None, family_alpha: float = 0.02, practical_delta: float = 0.03,
                delta_equivalence: float | None = None, min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None):
    """The pair table of the inference: the columns of ``_pairwise_estimates`` that are computed (see the module docstring for the
    ones left out), from ``rows`` of ``Engine.rr_inference`` or ``infer``.  A value the reference leaves None is null here too."""
    import pandas as pd

    rows = np.asarray(rows, dtype=RR_PAIR_ROW_DTYPE)
    n = int(n if n is not None else (len(strategy_ids) if strategy_ids is not None else (int(rows["strategy_b"].max()) + 1 if len(rows) else 0)))
    ids = _ids(strategy_ids, n)
    family = pair_count(n) if family_pair_count is None else int(family_pair_count)
    flags = rows["flags"]
    performed = (flags & FLAG_INFERENTIAL) != 0

    def only_tested(name: str):  # integer counts the reference reports only for a pair with a test
        return pd.array([int(x) if ok else None for x, ok in zip(rows[name], performed)], dtype="Int64")

    with np.errstate(divide="ignore", invalid="ignore"):
        descriptive_rate = rows["balanced_a_wins"] / (rows["n_ab"] + rows["n_ba"])
    frame = pd.DataFrame({
        "pair_id": rows["pair_id"].astype(np.int64),
        "strategy_a": ids[rows["strategy_a"]],
        "strategy_b": ids[rows["strategy_b"]],
        "games_attempted": rows["games_attempted"],
        "games_completed": rows["games_completed"],
        "games_safety_limit": rows["games_safety_limit"],
        "completion_game_rate": rows["completion_game_rate"],
        "n_completed_required": rows["n_completed_required"],
        "pair_inferentially_viable": performed,
        "pair_operationally_viable": (flags & FLAG_OPERATIONAL) != 0,
        "pair_claim_eligible": (flags & FLAG_ELIGIBLE) != 0,
        "completion_status": np.where(performed, "complete", "unresolved_nonviable"),
        "min_candidate_completion_rate": float(min_candidate_completion_rate),
        "n_ab": only_tested("n_ab"),
        "n_ba": only_tested("n_ba"),
        "seat1_a_wins_ab": only_tested("seat1_a_wins_ab"),
        "seat1_b_wins_ba": only_tested("seat1_b_wins_ba"),
        "seat2_a_wins_ba": only_tested("seat2_a_wins_ba"),
        "descriptive_a_wins_completed": rows["balanced_a_wins"],
        "descriptive_completed_games": rows["n_ab"] + rows["n_ba"],
        "descriptive_a_completed_win_rate": descriptive_rate,
        "q_ab": rows["q_ab"],
        "q_ba": rows["q_ba"],
        "raw_order_rate_difference": rows["raw_order_rate_difference"],
        "d_ab": rows["d_ab"],
        "score_null_proportion": rows["score_null_proportion"],
        "score_z": rows["score_z"],
        "score_p_value": rows["score_p_value"],
        "ordinary_alpha": float(family_alpha),
        "ordinary_d_low": rows["ordinary_d_low"],
        "ordinary_d_high": rows["ordinary_d_high"],
        "bonferroni_alpha_per_pair": float(family_alpha) / family if family else math.nan,
        "simultaneous_d_low": rows["simultaneous_d_low"],
        "simultaneous_d_high": rows["simultaneous_d_high"],
        "balanced_a_wins": only_tested("balanced_a_wins"),
        "balanced_total_games": pd.array([int(a + b) if ok else None for a, b, ok in zip(rows["n_ab"], rows["n_ba"], performed)], dtype="Int64"),
        "balanced_a_win_rate_alias": rows["balanced_a_win_rate"],
        "formal_test_performed": performed,
        "multiplicity_family_member": True,
        "no_test_p_value_convention": np.where(performed, None, "null_reported_treated_as_one_for_holm"),
        "holm_order": pd.array([int(x) if ok else None for x, ok in zip(rows["holm_order"], performed)], dtype="Int64"),
        "holm_adjusted_p": rows["holm_adjusted_p"],
        "holm_reject_before_viability": (flags & FLAG_REJECT_BEFORE) != 0,
        "holm_reject": (flags & FLAG_REJECT) != 0,
        "practical_delta": float(practical_delta),
        "delta_equivalence": math.nan if delta_equivalence is None else float(delta_equivalence),
        "equivalence_enabled": delta_equivalence is not None,
        "decision_class": np.asarray(DECISION_CLASSES, dtype=object)[rows["decision_class"]],
        "multiplicity_method": "holm",
    })
    return frame


def with_plan_columns(frame, target_power: float, worst_scenario_power: float):
    """``pairs_frame`` with the three columns the reference takes from its power plan (``_pairwise_estimates`` :808-816): the plan's
    target power, its worst-scenario power at the planned size, and whether the pair reached the completed support both are
    conditional on (its inferential viability)."""
    frame = frame.copy()
    frame["planned_target_power_conditional_on_completed_support"] = float(target_power)
    frame["planned_worst_scenario_power_conditional_on_completed_support"] = float(worst_scenario_power)
    frame["power_support_status"] = np.where(frame["pair_inferentially_viable"].to_numpy(dtype=bool), "completed_support_achieved",
                                             "unresolved_required_completed_support_not_achieved")
    return frame


def strategies_frame(strategies: np.ndarray, strategy_ids=None, min_candidate_completion_rate: float = 0.99):
    """The per-strategy table: the viability status of ``_viability_status`` (:679-698) and the class counts."""
    import pandas as pd

    st = np.asarray(strategies, dtype=np.int64)
    if st.ndim != 2 or st.shape[1] != RR_STRATEGY_COLS:
        raise ValueError(f"strategies must have shape (n, {RR_STRATEGY_COLS})")
    ids = _ids(strategy_ids, st.shape[0])
    attempted, completed, safety = st[:, 7], st[:, 8], st[:, 9]
    operational, inferential = st[:, 10] != 0, st[:, 11] != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        frame = pd.DataFrame({
            "strategy": ids,
            "games_attempted": attempted,
            "games_completed": completed,
            "games_safety_limit": safety,
            "completion_rate": completed / attempted,
            "safety_limit_rate": safety / attempted,
            "min_candidate_completion_rate": float(min_candidate_completion_rate),
            "operationally_viable": operational,
            "inferentially_viable": inferential,
            "candidate_status": np.where(operational & inferential, "viable",
                                         np.where(~operational, "operationally_nonviable", "inferentially_nonviable")),
        })
    for c, name in enumerate(STRATEGY_CLASS_COLS[:RR_CLASSES]):
        frame[name] = st[:, c]
    return frame
