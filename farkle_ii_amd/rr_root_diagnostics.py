"""Round-robin inference per root: the fixed-root diagnostics and the cross-root agreement.

``Engine.rr_root_diagnostics`` (``fk_rr_root_diagnostics``) runs ``_root_specific_diagnostics`` of the reference's
``src/farkle/analysis/h2h_inference.py`` (:918-1059) over root states that stay on the device (option ``"rr_keep_roots"``).  This
module is the host side:

* ``diagnose`` — the host statement of the entry, NumPy on ``rr_inference``'s ``combine_counts`` / ``viability`` / ``score_test`` /
  ``score_interval`` / ``holm_adjust``, returning what ``Engine.rr_root_diagnostics`` returns; the tests compare the two;
* ``root_pairs_frame`` / ``agreement_frame`` — ``root_pairwise_diagnostics.parquet`` and ``root_decision_agreement.parquet`` as
  ``farkle round-robin --inference --root-diagnostics`` writes them, columns named as the reference names them;
* ``stability_summary`` — ``root_specific_h2h_stability`` of the reference's ``structure_agreement.py`` (:205-215).

Each root is tested on its own counts with the COMBINED viability (:937-943): a pair that another root's block makes nonviable has no
test in any root, and operational viability is the all-roots completion rate.  Holm's family is every pair of the range, per root.
``root_a`` is the root with the smaller seed, whatever order the roots were played in.

Left out of the frames, as ``rr_inference.pairs_frame`` leaves them out: ``family_hash``, ``replacement_attempt_count``,
``score_test_id``, ``interval_method_id``.  ``root_seed`` / ``root_a`` / ``root_b`` are unsigned 64-bit (a seed may use the top bit);
the agreement columns the reference leaves None are null.
"""
from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from . import rr_inference as ri
from .backend import RR_AGREE_COLS, RR_AGREEMENT_ROW_DTYPE, RR_MAX_ROOTS, RR_ROOT_ROW_DTYPE
from .round_robin import pair_count

DIAGNOSTIC_DECISIONS = ("diagnostic_no_adjusted_rejection", "diagnostic_advantage_a", "diagnostic_advantage_b")  # FK_RR_DIAGNOSTIC_*
DECISION_NONE = 255  # FK_RR_DIAGNOSTIC_NONE
AGREE_AVAILABLE, AGREE_DECISION, AGREE_DIRECTION = 1, 2, 4  # FK_RR_AGREE_*
SUMMARY_COLS = ("pairs", "agreement_available", "decision_agreements", "direction_agreements") + tuple(
    f"root_{r}_{name}" for r in ("a", "b") for name in ("no_adjusted_rejection", "advantage_a", "advantage_b", "tests_performed"))  # FK_RR_AGREE_COLS
INFERENCE_ROLE = "fixed_root_diagnostic_not_root_population"
ROOT_PAIR_COLUMNS = ("root_seed", "pair_id", "strategy_a", "strategy_b", "n_ab", "n_ba", "games_attempted", "games_completed",
                     "games_safety_limit", "completion_game_rate", "completion_status", "pair_inferentially_viable",
                     "pair_operationally_viable", "pair_claim_eligible", "seat1_a_wins_ab", "seat1_b_wins_ba", "q_ab", "q_ba", "d_ab",
                     "score_null_proportion", "score_z", "score_p_value", "ordinary_alpha", "ordinary_d_low", "ordinary_d_high", "holm_order",
                     "holm_adjusted_p", "holm_reject", "diagnostic_holm_decision", "inference_role")
AGREEMENT_COLUMNS = ("pair_id", "strategy_a", "strategy_b", "root_a", "root_a_d_ab", "root_a_diagnostic_holm_decision", "root_b",
                     "root_b_d_ab", "root_b_diagnostic_holm_decision", "effect_discrepancy_a_minus_b", "absolute_effect_discrepancy",
                     "diagnostic_holm_decision_agreement", "effect_direction_agreement", "agreement_available", "interpretation")


def check_roots(root_seeds: Sequence[int]) -> list[int]:
    """One or two distinct roots (h2h_schedule.py:455-462), each an unsigned 64-bit seed."""
    seeds = [int(r) for r in root_seeds]
    if not 1 <= len(seeds) <= RR_MAX_ROOTS:
        raise ValueError(f"the root diagnostics admit one or two roots, got {len(seeds)}")
    if len(set(seeds)) != len(seeds):
        raise ValueError(f"the roots must be distinct, got {seeds}")
    if any(not 0 <= r < 1 << 64 for r in seeds):
        raise ValueError("a root seed must fit 64 unsigned bits")
    return seeds


def diagnose(n: int, root_states: Sequence[Any], root_seeds: Sequence[int], targets: Sequence[int], max_attempts: Sequence[int],
             pair_begin: int = 0, family_alpha: float = 0.02, practical_delta: float = 0.03, delta_equivalence: float | None = None,
             min_candidate_completion_rate: float = 0.99, family_pair_count: int | None = None, rows: tuple[int, int] | None = None,
             intervals: str = "brentq") -> dict:
    """The host statement of ``fk_rr_root_diagnostics``: ``root_states[r]`` are the block states ``[pairs, 2, 5]`` of root
    ``root_seeds[r]`` over pairs ``[pair_begin, pair_begin + pairs)`` of an ``n``-row table, in any order.  Returns ``{"roots", "rows"
    [n_roots, k], "agreement" [k], "summary", "max_abs_discrepancy"}`` as ``Engine.rr_root_diagnostics`` does (every pair of the range
    unless a pair-id range ``rows`` is given).  ``intervals`` as ``rr_inference.infer``."""
    if intervals not in ("brentq", "bisection"):
        raise ValueError(f"intervals must be 'brentq' or 'bisection', got {intervals!r}")
    seeds = check_roots(root_seeds)
    counts = ri.combine_counts(root_states, targets, max_attempts)
    n, begin, n_pairs = int(n), int(pair_begin), counts.shape[0]
    family = pair_count(n) if family_pair_count is None else int(family_pair_count)
    ri.check_params(n_pairs, family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family)
    status = ri.viability(n, counts, begin, min_candidate_completion_rate)
    pid, i, j, viable = status["pair_id"], status["i"], status["j"], status["viable"]
    pair_operational = status["operational"][i] & status["operational"][j]
    eligible = viable & pair_operational
    wanted = np.ones(n_pairs, dtype=bool) if rows is None else (pid >= int(rows[0])) & (pid < int(rows[1]))
    crit_ordinary, _ = ri.critical_values(family_alpha, family)
    v = np.flatnonzero(viable)

    order = sorted(range(len(seeds)), key=lambda r: seeds[r])  # ascending seed
    out = np.zeros((len(seeds), n_pairs), dtype=RR_ROOT_ROW_DTYPE)
    summary = np.zeros(RR_AGREE_COLS, dtype=np.int64)
    for slot, r in enumerate(order):
        st = np.asarray(root_states[r]).astype(np.int64)
        ab, ba = st[:, 0], st[:, 1]
        row = out[slot]
        row["pair_id"], row["strategy_a"], row["strategy_b"] = pid, i, j
        for c, name in enumerate(("games_attempted", "games_completed", "games_safety_limit")):
            row[name] = ab[:, c] + ba[:, c]
        n_ab, n_ba, x_ab, x_ba = ab[:, 1], ba[:, 1], ab[:, 3], ba[:, 3]
        row["n_ab"], row["n_ba"], row["seat1_a_wins_ab"], row["seat1_b_wins_ba"] = n_ab, n_ba, x_ab, x_ba
        with np.errstate(divide="ignore", invalid="ignore"):
            row["completion_game_rate"] = row["games_completed"] / row["games_attempted"]
        for name in ("q_ab", "q_ba", "d_ab", "score_null_proportion", "score_z", "score_p_value", "ordinary_d_low", "ordinary_d_high",
                     "holm_adjusted_p"):
            row[name] = np.nan
        if len(v):
            difference, null_proportion, z, p = ri.score_test(x_ab[v], n_ab[v], x_ba[v], n_ba[v])
            row["q_ab"][v], row["q_ba"][v] = x_ab[v] / n_ab[v], x_ba[v] / n_ba[v]
            row["d_ab"][v], row["score_null_proportion"][v], row["score_z"][v], row["score_p_value"][v] = 0.5 * difference, null_proportion, z, p
            idx = v[wanted[v]]
            if intervals == "bisection":
                low, high = ri.score_interval_many(x_ab[idx], n_ab[idx], x_ba[idx], n_ba[idx], crit_ordinary)
            else:  # the plain loop
                both = [ri.score_interval(int(x_ab[q]), int(n_ab[q]), int(x_ba[q]), int(n_ba[q]), crit_ordinary) for q in idx]
                low, high = (np.array([b[k] for b in both], dtype=np.float64) for k in (0, 1))
            row["ordinary_d_low"][idx], row["ordinary_d_high"][idx] = 0.5 * low, 0.5 * high
        adjusted, positions = ri.holm_adjust(np.where(viable, np.nan_to_num(row["score_p_value"], nan=1.0), 1.0))
        row["holm_order"] = np.where(viable, positions, 0)
        row["holm_adjusted_p"] = np.where(viable, adjusted, np.nan)
        reject_before = viable & (adjusted <= float(family_alpha))
        reject = reject_before & eligible
        row["flags"] = (viable * ri.FLAG_INFERENTIAL + pair_operational * ri.FLAG_OPERATIONAL + eligible * ri.FLAG_ELIGIBLE
                        + reject_before * ri.FLAG_REJECT_BEFORE + reject * ri.FLAG_REJECT).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            decision = np.where(reject, np.where(row["d_ab"] > 0.0, 1, 2), 0).astype(np.uint8)  # :945-953
        row["diagnostic_decision"] = decision
        summary[4 + 4 * slot: 7 + 4 * slot] = np.bincount(decision, minlength=3)
        summary[7 + 4 * slot] = viable.sum()

    agreement = np.zeros(n_pairs, dtype=RR_AGREEMENT_ROW_DTYPE)
    agreement["pair_id"], agreement["strategy_a"], agreement["strategy_b"] = pid, i, j
    agreement["root_a_d_ab"], agreement["root_a_decision"] = out[0]["d_ab"], out[0]["diagnostic_decision"]
    for name in ("root_b_d_ab", "effect_discrepancy_a_minus_b", "absolute_effect_discrepancy"):
        agreement[name] = np.nan
    agreement["root_b_decision"] = DECISION_NONE
    largest = float("nan")
    if len(seeds) == 2:
        a, b = out[0]["d_ab"], out[1]["d_ab"]
        available = ~np.isnan(a) & ~np.isnan(b)
        agreement["root_b_d_ab"], agreement["root_b_decision"] = b, out[1]["diagnostic_decision"]
        with np.errstate(invalid="ignore"):
            discrepancy = np.where(available, a - b, np.nan)
            direction = available & (np.sign(a) == np.sign(b))  # a zero effect has sign 0 and agrees only with another zero
        agreement["effect_discrepancy_a_minus_b"], agreement["absolute_effect_discrepancy"] = discrepancy, np.abs(discrepancy)
        same = available & (out[0]["diagnostic_decision"] == out[1]["diagnostic_decision"])
        agreement["flags"] = (available * AGREE_AVAILABLE + same * AGREE_DECISION + direction * AGREE_DIRECTION).astype(np.uint8)
        summary[1], summary[2], summary[3] = available.sum(), same.sum(), direction.sum()
        if available.any():
            largest = float(np.abs(discrepancy[available]).max())
    summary[0] = n_pairs
    return {"roots": np.array([seeds[r] for r in order], dtype=np.uint64), "rows": np.ascontiguousarray(out[:, wanted]),
            "agreement": agreement[wanted], "summary": summary, "max_abs_discrepancy": largest}


def _nullable_int(values, present) -> Any:
    import pandas as pd

    return pd.array([int(x) if ok else None for x, ok in zip(values, present)], dtype="Int64")


def root_pairs_frame(rows: np.ndarray, roots: Sequence[int], strategy_ids=None, n: int | None = None, family_alpha: float = 0.02):
    """``root_pairwise_diagnostics``: one row per (pair, root), sorted by pair and root seed (:995-997), the columns of :957-992 that
    are computed, from ``rows`` ``[n_roots, k]`` of ``Engine.rr_root_diagnostics`` or ``diagnose``."""
    import pandas as pd

    rows = np.asarray(rows, dtype=RR_ROOT_ROW_DTYPE)
    seeds = np.asarray([int(r) for r in roots], dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[0] != len(seeds):
        raise ValueError(f"rows must have shape (n_roots, pairs) for the {len(seeds)} roots, got {rows.shape}")
    k = rows.shape[1]
    root_seed = np.repeat(seeds[None, :], k, axis=0).reshape(-1)
    rows = np.ascontiguousarray(rows.T).reshape(-1)  # (pair, root) order; the roots ascend already
    n = int(n if n is not None else (len(strategy_ids) if strategy_ids is not None else (int(rows["strategy_b"].max()) + 1 if len(rows) else 0)))
    ids = ri._ids(strategy_ids, n)
    flags = rows["flags"]
    performed = (flags & ri.FLAG_INFERENTIAL) != 0
    frame = pd.DataFrame({
        "root_seed": root_seed,
        "pair_id": rows["pair_id"].astype(np.int64),
        "strategy_a": ids[rows["strategy_a"]],
        "strategy_b": ids[rows["strategy_b"]],
        "n_ab": _nullable_int(rows["n_ab"], performed),
        "n_ba": _nullable_int(rows["n_ba"], performed),
        "games_attempted": rows["games_attempted"],
        "games_completed": rows["games_completed"],
        "games_safety_limit": rows["games_safety_limit"],
        "completion_game_rate": rows["completion_game_rate"],
        "completion_status": np.where(performed, "complete", "unresolved_nonviable"),
        "pair_inferentially_viable": performed,
        "pair_operationally_viable": (flags & ri.FLAG_OPERATIONAL) != 0,
        "pair_claim_eligible": (flags & ri.FLAG_ELIGIBLE) != 0,
        "seat1_a_wins_ab": _nullable_int(rows["seat1_a_wins_ab"], performed),
        "seat1_b_wins_ba": _nullable_int(rows["seat1_b_wins_ba"], performed),
        "q_ab": rows["q_ab"],
        "q_ba": rows["q_ba"],
        "d_ab": rows["d_ab"],
        "score_null_proportion": rows["score_null_proportion"],
        "score_z": rows["score_z"],
        "score_p_value": rows["score_p_value"],
        "ordinary_alpha": float(family_alpha),
        "ordinary_d_low": rows["ordinary_d_low"],
        "ordinary_d_high": rows["ordinary_d_high"],
        "holm_order": _nullable_int(rows["holm_order"], performed),
        "holm_adjusted_p": rows["holm_adjusted_p"],
        "holm_reject": (flags & ri.FLAG_REJECT) != 0,
        "diagnostic_holm_decision": np.asarray(DIAGNOSTIC_DECISIONS, dtype=object)[rows["diagnostic_decision"]],
        "inference_role": INFERENCE_ROLE,
    })
    return frame[list(ROOT_PAIR_COLUMNS)]


def agreement_frame(agreement: np.ndarray, roots: Sequence[int], strategy_ids=None, n: int | None = None):
    """``root_decision_agreement``: one row per pair (:1003-1057) from ``agreement`` of ``Engine.rr_root_diagnostics`` or ``diagnose``."""
    import pandas as pd

    rows = np.asarray(agreement, dtype=RR_AGREEMENT_ROW_DTYPE)
    seeds = check_roots(roots)
    if seeds != sorted(seeds):
        raise ValueError(f"the roots come in ascending order, got {seeds}")
    n = int(n if n is not None else (len(strategy_ids) if strategy_ids is not None else (int(rows["strategy_b"].max()) + 1 if len(rows) else 0)))
    ids = ri._ids(strategy_ids, n)
    k, two = len(rows), len(seeds) == 2
    available = (rows["flags"] & AGREE_AVAILABLE) != 0
    names = np.asarray(DIAGNOSTIC_DECISIONS, dtype=object)

    def where_available(bit: int):
        return pd.array([bool(f & bit) if ok else None for f, ok in zip(rows["flags"], available)], dtype="boolean")

    frame = pd.DataFrame({
        "pair_id": rows["pair_id"].astype(np.int64),
        "strategy_a": ids[rows["strategy_a"]],
        "strategy_b": ids[rows["strategy_b"]],
        "root_a": np.full(k, seeds[0], dtype=np.uint64),
        "root_a_d_ab": rows["root_a_d_ab"],
        "root_a_diagnostic_holm_decision": names[rows["root_a_decision"]],
        "root_b": pd.array([seeds[1] if two else None] * k, dtype="UInt64"),
        "root_b_d_ab": rows["root_b_d_ab"],
        "root_b_diagnostic_holm_decision": names[rows["root_b_decision"]] if two else np.full(k, None, dtype=object),
        "effect_discrepancy_a_minus_b": rows["effect_discrepancy_a_minus_b"],
        "absolute_effect_discrepancy": rows["absolute_effect_discrepancy"],
        "diagnostic_holm_decision_agreement": where_available(AGREE_DECISION),
        "effect_direction_agreement": where_available(AGREE_DIRECTION),
        "agreement_available": available,
        "interpretation": np.where(available, "fixed_root_reproducibility_diagnostic_not_population_inference",
                                   "unavailable_for_unresolved_nonviable_pair") if two
        else np.full(k, "single_root_diagnostic_no_cross_root_stability_claim", dtype=object),
    })
    return frame[list(AGREEMENT_COLUMNS)]


def stability_summary(summary) -> dict:
    """``root_specific_h2h_stability`` (structure_agreement.py:205-215) from the entry's ``summary``: the fractions are agreements over
    the pairs with an agreement available, None when there is none."""
    s = np.asarray(summary, dtype=np.int64)
    if s.shape != (RR_AGREE_COLS,):
        raise ValueError(f"summary must hold {RR_AGREE_COLS} counts")
    available = int(s[1])
    return {"available": available > 0, "pair_count": int(s[0]),
            "diagnostic_decision_agreement_fraction": int(s[2]) / available if available else None,
            "effect_direction_agreement_fraction": int(s[3]) / available if available else None,
            "interpretation": "fixed_root_reproducibility_not_root_population_inference"}
