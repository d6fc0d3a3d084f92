"""A literal restatement of ``_root_specific_diagnostics`` of the reference's ``src/farkle/analysis/h2h_inference.py`` (:918-1059), and
of the parts of ``_viability_status`` (:638-700) and ``_pairwise_estimates`` (:717-881) it runs per root, for the tests of the
per-root diagnostics: plain Python, one loop per pair, dictionaries for rows, the statistics of ``rr_inference_literal``.  Nothing here
is shared with ``farkle_ii_amd.rr_root_diagnostics`` or the device header: the three are compared with each other."""
from __future__ import annotations

import math
from itertools import combinations

import numpy as np

import rr_inference_literal as lit


def block_rows(n, root_states, root_seeds, targets, max_attempts, pair_begin=0):
    """The raw count rows the reference reads: one per (pair, root, order)."""
    pairs = list(combinations(range(n), 2))
    out = []
    for states, root, target, cap in zip(root_states, root_seeds, targets, max_attempts):
        for k, both in enumerate(np.asarray(states).tolist()):
            a, b = pairs[pair_begin + k]
            for order, (attempted, completed, safety, wins1, wins2) in enumerate(both):
                out.append({"root_seed": int(root), "pair_id": pair_begin + k, "strategy_a": a, "strategy_b": b, "order": order,
                            "n_completed_required": int(target), "max_attempts": int(cap), "games_attempted": attempted,
                            "games_completed": completed, "games_safety_limit": safety, "wins_a": wins1 if order == 0 else wins2,
                            "wins_b": wins2 if order == 0 else wins1,
                            "completion_status": "complete" if completed >= target else "unresolved_nonviable"})
    return out


def viability_status(counts, threshold):
    """:644-699 -> (pair_viable, candidate_status)"""
    pair_viable = {}
    for row in counts:
        ok = row["completion_status"] == "complete" and row["games_completed"] == row["n_completed_required"]
        pair_viable[row["pair_id"]] = pair_viable.get(row["pair_id"], True) and ok
    status = {}
    for row in counts:
        for strategy in (row["strategy_a"], row["strategy_b"]):
            s = status.setdefault(strategy, {"games_attempted": 0, "games_completed": 0, "pairs": set()})
            s["games_attempted"] += row["games_attempted"]
            s["games_completed"] += row["games_completed"]
            s["pairs"].add(row["pair_id"])
    for s in status.values():
        rate = s["games_completed"] / s["games_attempted"] if s["games_attempted"] else None
        s["inferentially_viable"] = all(pair_viable[p] for p in s["pairs"])
        s["operationally_viable"] = rate is not None and rate >= threshold
    return pair_viable, status


def pairwise_estimates(selected, pair_viable, candidate_status, alpha, interval_every=1):
    """:717-881 on one root's rows (``_combine_within_order`` with one root changes no count): the columns the diagnostics keep.
    ``interval_every``: the brentq interval is slow, a large family computes it for the pair ids divisible by this (None elsewhere)."""
    by_pair = {}
    for row in selected:
        by_pair.setdefault(row["pair_id"], {})[row["order"]] = row
    rows = []
    for pair_id in sorted(by_pair):
        ab, ba = by_pair[pair_id][0], by_pair[pair_id][1]
        n_ab, n_ba = ab["games_completed"], ba["games_completed"]
        x_ab, x_ba = ab["wins_a"], ba["wins_b"]
        viable = pair_viable[pair_id]
        if viable and n_ab != n_ba:
            raise ValueError(f"pair {pair_id} is not exactly balanced between seat orders")
        operational = bool(candidate_status[ab["strategy_a"]]["operationally_viable"] and candidate_status[ab["strategy_b"]]["operationally_viable"])
        attempted = ab["games_attempted"] + ba["games_attempted"]
        row = {"pair_id": pair_id, "strategy_a": ab["strategy_a"], "strategy_b": ab["strategy_b"], "games_attempted": attempted,
               "games_completed": n_ab + n_ba, "games_safety_limit": ab["games_safety_limit"] + ba["games_safety_limit"],
               "completion_game_rate": (n_ab + n_ba) / attempted, "pair_inferentially_viable": viable,
               "pair_operationally_viable": operational, "pair_claim_eligible": viable and operational,
               "completion_status": "complete" if viable else "unresolved_nonviable",
               "n_ab": n_ab if viable else None, "n_ba": n_ba if viable else None, "seat1_a_wins_ab": x_ab if viable else None,
               "seat1_b_wins_ba": x_ba if viable else None, "q_ab": None, "q_ba": None, "d_ab": None, "score_null_proportion": None,
               "score_z": None, "score_p_value": None, "ordinary_d_low": None, "ordinary_d_high": None, "formal_test_performed": viable}
        if viable:
            difference, pooled, stat, p = lit.score_test(x_ab, n_ab, x_ba, n_ba)
            row.update({"q_ab": x_ab / n_ab, "q_ba": x_ba / n_ba, "d_ab": 0.5 * difference, "score_null_proportion": pooled, "score_z": stat,
                        "score_p_value": p})
            if pair_id % interval_every == 0:
                low, high = lit.interval(x_ab, n_ab, x_ba, n_ba, alpha)
                row.update({"ordinary_d_low": 0.5 * low, "ordinary_d_high": 0.5 * high})
        rows.append(row)
    working = np.array([r["score_p_value"] if r["formal_test_performed"] and r["score_p_value"] is not None else 1.0 for r in rows], dtype=float)
    adjusted, positions = lit.holm(working)
    for r, adj, place in zip(rows, adjusted, positions):
        performed = r["formal_test_performed"]
        r["holm_order"] = int(place) if performed else None
        r["holm_adjusted_p"] = float(adj) if performed else math.nan
        r["holm_reject_before_viability"] = bool(performed and adj <= alpha)
        r["holm_reject"] = r["holm_reject_before_viability"] and r["pair_claim_eligible"]
    return rows


def root_specific_diagnostics(n, root_states, root_seeds, targets, max_attempts, pair_begin=0, family_alpha=0.02,
                              min_candidate_completion_rate=0.99, interval_every=1):
    """:928-1059 -> (diagnostics, agreement): lists of dictionaries, the first sorted by (pair_id, root_seed)."""
    counts = block_rows(n, root_states, root_seeds, targets, max_attempts, pair_begin)
    pair_viable, candidate_status = viability_status(counts, float(min_candidate_completion_rate))
    diagnostics = []
    for root in [int(r) for r in root_seeds]:
        selected = [row for row in counts if row["root_seed"] == root]
        for row in pairwise_estimates(selected, pair_viable, candidate_status, family_alpha, interval_every):
            row["root_seed"] = root
            d_ab = math.nan if row["d_ab"] is None else row["d_ab"]
            if row["holm_reject"]:
                row["diagnostic_holm_decision"] = "diagnostic_advantage_a" if d_ab > 0.0 else "diagnostic_advantage_b"
            else:
                row["diagnostic_holm_decision"] = "diagnostic_no_adjusted_rejection"
            diagnostics.append(row)
    diagnostics.sort(key=lambda r: (r["pair_id"], r["root_seed"]))
    groups = {}
    for r in diagnostics:  # (sorted by root_seed within a pair already)
        groups.setdefault(r["pair_id"], []).append(r)
    rows = []
    for pair_id in sorted(groups):
        ordered = groups[pair_id]
        first = ordered[0]
        row = {"pair_id": pair_id, "strategy_a": first["strategy_a"], "strategy_b": first["strategy_b"], "root_a": first["root_seed"],
               "root_a_d_ab": first["d_ab"], "root_a_diagnostic_holm_decision": first["diagnostic_holm_decision"], "root_b": None,
               "root_b_d_ab": None, "root_b_diagnostic_holm_decision": None, "effect_discrepancy_a_minus_b": None,
               "absolute_effect_discrepancy": None, "diagnostic_holm_decision_agreement": None, "effect_direction_agreement": None,
               "agreement_available": False, "interpretation": "single_root_diagnostic_no_cross_root_stability_claim"}
        if len(ordered) == 2:
            second = ordered[1]
            first_effect, second_effect = first["d_ab"], second["d_ab"]
            both = first_effect is not None and second_effect is not None
            discrepancy = first_effect - second_effect if both else None
            row.update({"root_b": second["root_seed"], "root_b_d_ab": second_effect,
                        "root_b_diagnostic_holm_decision": second["diagnostic_holm_decision"],
                        "effect_discrepancy_a_minus_b": discrepancy,
                        "absolute_effect_discrepancy": None if discrepancy is None else abs(discrepancy),
                        "diagnostic_holm_decision_agreement": (first["diagnostic_holm_decision"] == second["diagnostic_holm_decision"]) if both else None,
                        "effect_direction_agreement": (int(np.sign(first_effect)) == int(np.sign(second_effect))) if both else None,
                        "agreement_available": both,
                        "interpretation": ("fixed_root_reproducibility_diagnostic_not_population_inference" if both
                                           else "unavailable_for_unresolved_nonviable_pair")})
        rows.append(row)
    return diagnostics, rows
