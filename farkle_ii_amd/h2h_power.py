"""The round robin's power plan: the block size at which the two-sided score test reaches its target power in every seat-advantage
scenario, found by scanning exact power on the device.

The reference's ``src/farkle/analysis/h2h_schedule.py`` sizes its blocks by the exact power of the score rule it implements
(``implemented_score_test_power`` :324-358), which is not monotone in the sample size, so it evaluates every block size from 1 upwards
(``_minimum_block_games`` :393-420) at every scenario.  ``Engine.score_power_scan`` (``fk_score_power_scan``) evaluates those
(sample size, scenario) cells in one launch per window of block sizes.  This module is the host side:

* ``boundaries`` — the rejecting count boundaries of every first-sample count (``_fixed_first_count_boundary_arrays`` :273-295), the
  NumPy statement the device's ``pp_boundaries`` (csrc/fk_power_plan.h) equals integer for integer;
* ``score_test_power`` — the exact host statement: the same ``scipy.stats.binom`` calls and the same dot product as the reference,
  hence its bits;
* ``power_cells_host`` — the NumPy statement of what the device computes (log-factorial table, prefix and suffix sums); the tests
  compare the device with it;
* ``plan_block_games`` — the scan: the device finds the block sizes whose worst-scenario power is within ``GUARD`` of the target or
  above it, ``score_test_power`` decides them in ascending order, so the plan is the reference's first crossing and the two reported
  powers are its bits;
* ``power_grid`` / ``plan_document`` / ``curve_frame`` — ``h2h_power_plan.json`` (the keys of the reference's plan this package can
  compute) and ``h2h_power_curve.parquet`` (one row per scanned block size, which the reference cannot afford to compute);
* ``independent_score_planning_power`` — the large-sample formula, host only.

Left out of the plan document: ``family_hash``, ``schedule_hash``, ``profile``, the schema and RNG version stamps, sidecars and the
stage stamp.  The conditional-Fisher cross-check the reference adds at ``n <= 64`` is not made.
"""
from __future__ import annotations

import functools
import math
from typing import Any, Sequence

import numpy as np

from .backend import POWER_CELL_DTYPE, POWER_MAX_N

SCORE_TEST_ID = "independent_two_proportion_score_v1"
POWER_METHOD_ID = "conditional_exact_power_first_crossing_v2"
H2H_METHOD_VERSION = 2
MAX_HOST_EVALUATIONS = 8  # block sizes of one plan the host statement may have to decide: a condition, not a measurement
DEFAULT_WINDOW = 256      # block sizes of one device call

# Tolerances of the two comparisons, measured and recorded as DESIGN 5.14 says (4 x the worst relative difference among cells whose
# power exceeds the absolute tolerance; the absolute tolerance is the reference's own 1e-13):
# power_cells_host against the reference's recorded powers (tests/golden/power_plan_vectors.json: "measured")
HOST_REL_TOL = 3.61e-11  # measured 9.0243e-12 at n = 20001, q = (0.59, 0.53), alpha = 0.02 / 13310220
HOST_ABS_TOL = 1e-13
# the device against power_cells_host (tests/test_power_plan_gpu.py prints the worst case)
DEVICE_REL_TOL = 6.7e-15  # measured 1.6653e-15 at n = 20001, q = (0.56, 0.5), alpha = 0.02 / 13310220 (MI355X)
DEVICE_ABS_TOL = 1e-13
GUARD = (HOST_REL_TOL + HOST_ABS_TOL) + (DEVICE_REL_TOL + DEVICE_ABS_TOL)  # both bounds at power 1: what a device value may be off by


class PowerPlanError(RuntimeError):
    """The search ended without a plan: no block size up to the entry's limit reaches the target, or the device scan left more block
    sizes undecided than the host statement is allowed to decide."""


def critical_value(alpha: float) -> float:
    """``norm.isf(alpha / 2)``: the two-sided critical value of the score statistic."""
    from scipy.stats import norm

    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    return float(norm.isf(alpha / 2.0))


def scenario_probabilities(effect: float, seat1_advantage: float) -> tuple[float, float]:
    """``(q_ab, q_ba)`` of a reported half-difference ``effect`` under a common seat-1 advantage (``_scenario_probabilities``)."""
    q_ab = 0.5 + seat1_advantage + effect
    q_ba = 0.5 + seat1_advantage - effect
    if not 0.0 < q_ba < q_ab < 1.0:
        raise ValueError(f"effect {effect} with seat-1 advantage {seat1_advantage} gives no valid probabilities: q_ab={q_ab}, q_ba={q_ba}")
    return q_ab, q_ba


def make_cells(n, q_ab, q_ba) -> np.ndarray:
    """``POWER_CELL_DTYPE`` cells from three broadcastable arrays."""
    n, q_ab, q_ba = np.broadcast_arrays(np.asarray(n), np.asarray(q_ab, dtype=np.float64), np.asarray(q_ba, dtype=np.float64))
    cells = np.zeros(n.size, dtype=POWER_CELL_DTYPE)
    cells["n"], cells["q_ab"], cells["q_ba"] = n.reshape(-1), q_ab.reshape(-1), q_ba.reshape(-1)
    return cells


def boundaries(n: int, critical: float) -> tuple[np.ndarray, np.ndarray]:
    """``(lower, upper)``, int64 ``[n + 1]``: for a first-sample count ``c1`` the test rejects exactly the second-sample counts
    ``<= lower[c1]`` and ``>= upper[c1]`` (``-1`` / ``n + 1``: none).  They are the roots in ``count2`` of
    ``n (c1 - c2)^2 = critical^2 (c1 + c2)(2n - c1 - c2) / 2``, the rejection being strict."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    c1 = np.arange(n + 1, dtype=np.float64)
    squared = float(critical) ** 2
    a = 2.0 * n + squared
    b = -4.0 * n * c1 - 2.0 * squared * (n - c1)
    c = a * c1 * c1 - 2.0 * squared * n * c1
    distance = np.sqrt(np.maximum(b * b - 4.0 * a * c, 0.0))
    low_root = (-b - distance) / (2.0 * a)
    high_root = (-b + distance) / (2.0 * a)
    lower = np.clip(np.ceil(low_root).astype(np.int64) - 1, -1, n)
    upper = np.clip(np.floor(high_root).astype(np.int64) + 1, 0, n + 1)
    lower[0] = -1
    upper[n] = n + 1
    return lower, upper


def _check_cell(n: int, q_ab: float, q_ba: float) -> None:
    if n < 1:
        raise ValueError("games per order must be positive")
    if not 0.0 < q_ab < 1.0 or not 0.0 < q_ba < 1.0:
        raise ValueError("probabilities must lie strictly between zero and one")


@functools.lru_cache(maxsize=4096)
def score_test_power(n: int, q_ab: float, q_ba: float, alpha: float) -> float:
    """Exact power of the score rule with ``n`` completed games per order: the probability, under independent ``Bin(n, q_ab)`` and
    ``Bin(n, q_ba)``, that the second count falls at or beyond a boundary of the first.  The reference's bits."""
    from scipy.stats import binom

    n = int(n)
    _check_cell(n, q_ab, q_ba)
    lower, upper = boundaries(n, critical_value(alpha))
    mass_first = binom.pmf(np.arange(n + 1, dtype=np.int64), n, q_ab)
    reject = binom.cdf(lower, n, q_ba) + binom.sf(upper - 1, n, q_ba)
    return min(1.0, max(0.0, float(np.dot(mass_first, reject))))


def independent_score_planning_power(n: int, q_ab: float, q_ba: float, alpha: float) -> float:
    """The large-sample power of the same test (normal approximation under the null and the alternative variance)."""
    from scipy.stats import norm

    _check_cell(int(n), q_ab, q_ba)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must be between zero and one")
    pooled = 0.5 * (q_ab + q_ba)
    sd_null = math.sqrt(2.0 * pooled * (1.0 - pooled) / n)
    sd_alt = math.sqrt((q_ab * (1.0 - q_ab) + q_ba * (1.0 - q_ba)) / n)
    edge = float(norm.ppf(1.0 - alpha / 2.0)) * sd_null
    gap = q_ab - q_ba
    return min(1.0, max(0.0, float(norm.sf((edge - gap) / sd_alt)) + float(norm.cdf((-edge - gap) / sd_alt))))


_LF = np.zeros(2, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _lgammal():
    """libm's long-double ``lgamma``: the call the library fills the device's table with (csrc/farkle_hip.hip: ``power_plan_table``)."""
    import ctypes
    import ctypes.util

    fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").lgammal
    fn.restype, fn.argtypes = ctypes.c_longdouble, [ctypes.c_longdouble]
    return fn


def log_factorials(n_max: int) -> np.ndarray:
    """``lf[k] = log k!`` for ``k = 0 .. n_max``: libm's long-double ``lgamma(k + 1)`` rounded to float64 — the table the device context
    keeps, entry for entry.  (``math.lgamma`` and the float64 ``lgamma`` of libm are each a few units in the last place off at
    ``k`` of order 10^4, and differently so; the exponent of a mass is of order 10^5 there.)"""
    global _LF
    if n_max + 1 > len(_LF):
        grown = np.zeros(max(n_max + 1, 2 * len(_LF)), dtype=np.float64)
        grown[: len(_LF)] = _LF
        lgammal = _lgammal()
        grown[len(_LF):] = [float(lgammal(k + 1.0)) for k in range(len(_LF), len(grown))]
        _LF = grown
    return _LF


def _masses(lf: np.ndarray, n: int, q: float) -> np.ndarray:
    k = np.arange(n + 1, dtype=np.int64)
    return np.exp(lf[n] - lf[k] - lf[n - k] + k * math.log(q) + (n - k) * math.log1p(-q))


def power_cells_host(cells, critical: float) -> np.ndarray:
    """What ``fk_score_power_scan`` computes, in NumPy: per cell the masses of both counts from the log-factorial table, the lower tail
    of the second count as a prefix sum and its upper tail as a suffix sum, gathered at ``boundaries``.  float64 ``[cells]``."""
    cells = np.ascontiguousarray(cells, dtype=POWER_CELL_DTYPE).reshape(-1)
    out = np.zeros(len(cells), dtype=np.float64)
    if not len(cells):
        return out
    if not math.isfinite(critical) or not critical > 0.0:
        raise ValueError(f"critical must be finite and positive, got {critical}")
    if cells["n"].min() < 1 or cells["n"].max() > POWER_MAX_N:
        raise ValueError(f"n must be in [1, {POWER_MAX_N}]")
    lf = log_factorials(int(cells["n"].max()))
    edges: dict = {}
    tails: dict = {}
    done: dict = {}
    for at, (n, _, q_ab, q_ba) in enumerate(cells.tolist()):
        if (n, q_ab, q_ba) in done:
            out[at] = done[n, q_ab, q_ba]
            continue
        _check_cell(n, q_ab, q_ba)
        if n not in edges:
            edges[n] = boundaries(n, critical)
        lower, upper = edges[n]
        if (n, q_ba) not in tails:
            mass = _masses(lf, n, q_ba)
            tails[n, q_ba] = (np.cumsum(mass), np.cumsum(mass[::-1])[::-1])
        below, above = tails[n, q_ba]
        reject = np.where(lower >= 0, below[np.maximum(lower, 0)], 0.0) + np.where(upper <= n, above[np.minimum(upper, n)], 0.0)
        out[at] = done[n, q_ab, q_ba] = min(1.0, max(0.0, float(np.dot(_masses(lf, n, q_ab), reject))))
    return out


def worst_scenario_power(block_games: int, root_count: int, effect: float, scenarios: Sequence[float], alpha_per_pair: float) -> float:
    """The smallest ``score_test_power`` over the scenarios at ``block_games x root_count`` games per order."""
    n = int(block_games) * int(root_count)
    return min(score_test_power(n, *scenario_probabilities(effect, float(s)), alpha_per_pair) for s in scenarios)


def plan_block_games(engine, *, root_count: int, effect: float, scenarios: Sequence[float], alpha_per_pair: float, target_power: float,
                     window: int = DEFAULT_WINDOW, guard: float = GUARD, max_host_evaluations: int = MAX_HOST_EVALUATIONS) -> dict:
    """The smallest block size whose worst-scenario exact power reaches ``target_power``: the reference's ``_minimum_block_games``.

    Block sizes are scanned in ascending windows, one ``engine.score_power_scan`` call of ``window x len(scenarios)`` cells each.  A
    size whose device worst power lies below ``target_power - guard`` cannot reach the target (``guard`` covers the device's error) and
    is passed over; every other size is decided by ``score_test_power``, in ascending order, and the first that reaches the target is
    the plan.  Returns ``block_games``, the two powers the reference reports (host statement: its bits), ``host_evaluations`` and
    ``curve`` — float64 ``[scanned sizes, 2 + len(scenarios) + 1]``: block size, games per order, device power per scenario, worst."""
    root_count, window = int(root_count), int(window)
    scenarios = tuple(float(s) for s in scenarios)
    if root_count < 1 or window < 1 or not scenarios:
        raise ValueError("a plan needs at least one root, one scenario and a window of at least one block size")
    if not 0.0 < target_power < 1.0:
        raise ValueError(f"target_power must be in (0, 1), got {target_power}")
    if not 0.0 < alpha_per_pair < 1.0:
        raise ValueError(f"alpha_per_pair must be in (0, 1), got {alpha_per_pair}")
    q = np.array([scenario_probabilities(effect, s) for s in scenarios], dtype=np.float64)
    limit = POWER_MAX_N // root_count
    curve, evaluated, first = [], 0, 1
    while first <= limit:
        blocks = np.arange(first, min(first + window, limit + 1), dtype=np.int64)
        cells = make_cells(np.repeat(blocks * root_count, len(scenarios)), np.tile(q[:, 0], len(blocks)), np.tile(q[:, 1], len(blocks)))
        power = np.asarray(engine.score_power_scan(cells, alpha_per_pair), dtype=np.float64).reshape(len(blocks), len(scenarios))
        worst = power.min(axis=1)
        curve.append(np.column_stack([blocks, blocks * root_count, power, worst]))
        for block in blocks[worst >= target_power - guard].tolist():
            evaluated += 1
            if evaluated > max_host_evaluations:
                raise PowerPlanError(f"power plan: more than {max_host_evaluations} block sizes lie within {guard:g} of the target power "
                                   f"{target_power!r} on the device (the last at block size {block}): the device scan does not separate them")
            achieved = worst_scenario_power(block, root_count, effect, scenarios, alpha_per_pair)
            if achieved >= target_power:
                previous = worst_scenario_power(block - 1, root_count, effect, scenarios, alpha_per_pair) if block > 1 else 0.0
                return {"block_games": block, "worst_scenario_achieved_power": achieved, "previous_equal_block_size_worst_power": previous,
                        "host_evaluations": evaluated, "curve": np.concatenate(curve), "scenarios": scenarios, "root_count": root_count}
        first += window
    raise PowerPlanError(f"power plan: no block size up to {limit} ({POWER_MAX_N} games per order over {root_count} roots) reaches the target "
                       f"power {target_power!r}")


def power_grid(block_games: int, root_count: int, sensitivity_deltas: Sequence[float], scenarios: Sequence[float],
               alpha_per_pair: float) -> list[dict]:
    """The plan document's ``power_validation``: the exact power at the planned size for every sensitivity effect and scenario."""
    n = int(block_games) * int(root_count)
    rows = []
    for effect in sensitivity_deltas:
        for advantage in scenarios:
            q_ab, q_ba = scenario_probabilities(float(effect), float(advantage))
            rows.append({"reported_effect": float(effect), "seat1_advantage": float(advantage), "q_ab": q_ab, "q_ba": q_ba, "games_per_order": n,
                         "power_conditioning": "exact_completed_games_per_order_achieved",
                         "achieved_power": score_test_power(n, q_ab, q_ba, alpha_per_pair)})
    return rows


def plan_from_config(engine, h2h, candidate_count: int, roots: Sequence[int], window: int = DEFAULT_WINDOW) -> dict:
    """``plan_block_games`` with the ``head2head`` settings ``h2h`` (``AppConfig.head2head``) for a family of ``candidate_count``
    strategies on ``roots``; the result also carries ``pair_count`` and ``alpha_per_pair``."""
    h2h.check_plan()
    roots = tuple(int(r) for r in roots)
    if len(roots) not in (1, 2) or len(set(roots)) != len(roots):
        raise ValueError(f"a power plan takes one or two distinct root seeds, got {list(roots)}")
    if len(roots) == 1 and not h2h.allow_single_root:
        raise ValueError("single-root H2H is disabled by head2head.allow_single_root")
    if candidate_count < 2:
        raise ValueError(f"a power plan needs at least two candidates, got {candidate_count}")
    pair_count = candidate_count * (candidate_count - 1) // 2
    alpha_per_pair = h2h.family_alpha / pair_count
    plan = plan_block_games(engine, root_count=len(roots), effect=h2h.practical_delta, scenarios=h2h.seat1_advantage_scenarios,
                            alpha_per_pair=alpha_per_pair, target_power=h2h.target_power, window=window)
    return {**plan, "candidate_count": int(candidate_count), "pair_count": pair_count, "alpha_per_pair": alpha_per_pair, "roots": roots}


def plan_document(plan: dict, h2h, max_attempt_multiplier: float) -> dict:
    """``h2h_power_plan.json`` from ``plan_from_config``'s result: the reference's plan keys that need no hash, profile or stamp."""
    multiplier = float(max_attempt_multiplier)
    if not math.isfinite(multiplier) or multiplier < 1.0:
        raise ValueError("head2head.max_attempt_multiplier must be finite and at least 1")
    block, roots, pairs = int(plan["block_games"]), tuple(plan["roots"]), int(plan["pair_count"])
    per_pair = block * len(roots) * 2
    attempts = math.ceil(multiplier * block)
    return {
        "candidate_count": int(plan["candidate_count"]),
        "unordered_pair_count": pairs,
        "root_seeds": list(roots),
        "single_root_execution": len(roots) == 1,
        "score_test_id": SCORE_TEST_ID,
        "power_method_id": POWER_METHOD_ID,
        "h2h_method_version": H2H_METHOD_VERSION,
        "test_direction": "two_sided",
        "final_multiplicity_method": "holm",
        "planning_multiplicity_method": "bonferroni",
        "family_alpha": h2h.family_alpha,
        "alpha_per_pair": plan["alpha_per_pair"],
        "target_power": h2h.target_power,
        "power_conditioning": "conditional_on_achieving_n_completed_required_in_every_pair_root_order_cell",
        "target_effect": h2h.practical_delta,
        "n_completed_required_per_root_order_block": block,
        "n_completed_required_per_order_across_roots": block * len(roots),
        "n_completed_required_per_pair": per_pair,
        "total_completed_required": per_pair * pairs,
        "max_attempt_multiplier": multiplier,
        "max_attempts_per_root_order_block": attempts,
        "maximum_total_attempts": attempts * len(roots) * 2 * pairs,
        "min_candidate_completion_rate": h2h.min_candidate_completion_rate,
        "total_block_count": pairs * len(roots) * 2,
        "worst_scenario_achieved_power": plan["worst_scenario_achieved_power"],
        "previous_equal_block_size_worst_power": plan["previous_equal_block_size_worst_power"],
        "power_validation": power_grid(block, len(roots), h2h.sensitivity_deltas, h2h.seat1_advantage_scenarios, plan["alpha_per_pair"]),
    }


def curve_frame(plan: dict) -> Any:
    """``h2h_power_curve.parquet``: one row per scanned block size — ``block_games``, ``games_per_order``, the device's power per
    scenario (``power_seat1_advantage_<value>``) and ``worst_scenario_power``."""
    import pandas as pd

    curve = np.asarray(plan["curve"], dtype=np.float64)
    data = {"block_games": curve[:, 0].astype(np.int64), "games_per_order": curve[:, 1].astype(np.int64)}
    for at, advantage in enumerate(plan["scenarios"]):
        data[f"power_seat1_advantage_{advantage:g}"] = curve[:, 2 + at]
    data["worst_scenario_power"] = curve[:, -1]
    return pd.DataFrame(data)

