"""Method agreement of a round robin: the reference's ``src/farkle/analysis/structure_agreement.py`` over the decision classes of
``rr_inference`` and the frozen candidate membership.

``Engine.agreement_pairs`` (``fk_agreement_pairs``) and ``Engine.rr_agreement`` (``fk_rr_agreement``) give every pair one code byte —
bits 0-1 ``h2h_direction``, 2-3 ``win_rate_preference``, 4-5 ``trueskill_preference``, each 0 none / 1 a / 2 b — and count what the
summary needs; ``Engine.rank_concordance`` (``fk_rank_concordance``) counts Kendall's concordant, discordant and tied pairs of the
scored population.  Every result is an integer.  This module is the host side:

* ``pair_codes`` / ``pair_counts`` / ``concordance_counts`` — the host statements of the three entries in NumPy; the tests compare
  device and host byte for byte;
* ``kendall_from_counts`` — scipy's tau-b from the integer counts, bit for bit; Spearman has no hot path and is scipy's on the host;
* ``read_membership`` / ``membership_from_frame`` — the reference's ``candidate_family.parquet`` (``candidate_family.py:364-433``),
  with its refusals (``_pair_agreement`` :76-83, ``_summary`` :163-165), and the two rank arrays in table order;
* ``pairs_frame`` / ``summary`` — ``selection_conditioned_pairs.parquet`` (``_pair_agreement`` :73-125) and
  ``agreement_summary.json`` (``_summary`` :133-216) in the reference's columns, dtypes, row order and keys.

The membership is caller-supplied: the candidate freeze and TrueSkill are not produced by this package.  Also left out: sidecars and
the stage stamp.
"""
from __future__ import annotations

from typing import Any

import numpy as np

from .backend import AGREE_COUNTS, AGREE_NO_RANK, CONCORDANCE_COUNTS, RR_CLASSES
from .round_robin import pair_count, pair_ids
from .rr_inference import DECISION_CLASSES

COUNT_NAMES = ("pairs", "directional", "unresolved", "unresolved_nonviable", "equivalent", "win_rate_trueskill_available", "win_rate_trueskill_agree",
               "h2h_win_rate_available", "h2h_win_rate_agree", "h2h_trueskill_available", "h2h_trueskill_agree")
CONCORDANCE_NAMES = ("concordant", "discordant", "tied_x_only", "tied_y_only", "tied_both")
MEMBERSHIP_FLAGS = ("scored_by_both_methods", "final_family", "initial_win_rate_contribution", "initial_trueskill_contribution",
                    "final_win_rate_contribution", "final_trueskill_contribution", "final_shared_contribution", "configured_control",
                    "mandatory_diagnostic")
MEMBERSHIP_COLUMNS = ("strategy", "win_rate_rank", "trueskill_rank", "family_hash", *MEMBERSHIP_FLAGS)
PAIR_COLUMNS = ("family_hash", "pair_id", "strategy_a", "strategy_b", "decision_class", "h2h_direction", "win_rate_preference", "trueskill_preference",
                "win_rate_trueskill_agree", "h2h_agrees_with_win_rate", "h2h_agrees_with_trueskill", "selection_conditioning")
SELECTION_CONDITIONING = "frozen_finite_grid_candidate_family"
CONDITIONING = "agreement_is_conditioned_on_the_frozen_finalist_family"
EXECUTION_SCOPES = {1: "single_root", 2: "root_pair"}


# ---- the host statements of the entries ----
def _ranks(values, n: int, what: str) -> np.ndarray:
    a = np.asarray(values, dtype=np.int64).reshape(-1)
    if len(a) != n:
        raise ValueError(f"{what} must name the {n} rows of the table")
    if len(a) and int(a.min()) < 0:
        raise ValueError(f"{what} holds a negative rank: a rank is at least 1, {AGREE_NO_RANK} is null")
    return a


def preference(rank_a: np.ndarray, rank_b: np.ndarray) -> np.ndarray:
    """``_preference`` (:55-62) on arrays: 0 none (a null rank, or equal ranks), 1 a (A's rank is the smaller), 2 b."""
    none = (rank_a == AGREE_NO_RANK) | (rank_b == AGREE_NO_RANK) | (rank_a == rank_b)
    return np.where(none, 0, np.where(rank_a < rank_b, 1, 2)).astype(np.uint8)


def pair_codes(n: int, decision_class, win_rate_rank, trueskill_rank) -> np.ndarray:
    """The host statement of ``fk_agreement_pairs``' codes: uint8 ``[n (n - 1) / 2]`` in pair-id order."""
    n = int(n)
    if n < 2:
        raise ValueError(f"pair agreement needs at least two strategies, got {n}")
    cls = np.asarray(decision_class, dtype=np.uint8).reshape(-1)
    if len(cls) != pair_count(n):
        raise ValueError(f"a table of {n} strategies has {pair_count(n)} pairs")
    if len(cls) and int(cls.max()) >= RR_CLASSES:
        raise ValueError(f"decision class {int(cls.max())} is not one of the {RR_CLASSES} classes")
    win, ts = _ranks(win_rate_rank, n, "win_rate_rank"), _ranks(trueskill_rank, n, "trueskill_rank")
    _, i, j = pair_ids(n)
    direction = np.where(cls < 4, 1 + (cls & 1), 0).astype(np.uint8)
    return direction | preference(win[i], win[j]) << 2 | preference(ts[i], ts[j]) << 4


def pair_counts(codes, decision_class) -> np.ndarray:
    """The host statement of ``fk_agreement_pairs``' counts (``COUNT_NAMES``) from the codes and the classes."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    cls = np.asarray(decision_class, dtype=np.uint8).reshape(-1)
    if len(codes) != len(cls):
        raise ValueError("one code and one class per pair")
    h, w, t = codes & 3, (codes >> 2) & 3, (codes >> 4) & 3
    each = (np.ones(len(codes), dtype=bool), h != 0, cls >= 5, cls == 6, cls == 4, (w != 0) & (t != 0), (w != 0) & (w == t), (h != 0) & (w != 0),
            (h != 0) & (h == w), (h != 0) & (t != 0), (h != 0) & (h == t))
    assert len(each) == AGREE_COUNTS
    return np.array([int(np.count_nonzero(e)) for e in each], dtype=np.int64)


def concordance_counts(x, y) -> np.ndarray:
    """The host statement of ``fk_rank_concordance``: int64 ``[5]`` (``CONCORDANCE_NAMES``) over all ``i < j``, one row against the
    items after it at a time."""
    x, y = np.asarray(x, dtype=np.int64).reshape(-1), np.asarray(y, dtype=np.int64).reshape(-1)
    if len(x) != len(y):
        raise ValueError("x and y must have one key per item each")
    if len(x) and (int(x.min()) < 1 or int(y.min()) < 1):
        raise ValueError("a key is at least 1")
    out = np.zeros(CONCORDANCE_COUNTS, dtype=np.int64)
    for i in range(len(x) - 1):
        tie_x, tie_y = x[i + 1:] == x[i], y[i + 1:] == y[i]
        same_way = (x[i] < x[i + 1:]) == (y[i] < y[i + 1:])
        free = ~tie_x & ~tie_y
        out += (np.count_nonzero(free & same_way), np.count_nonzero(free & ~same_way), np.count_nonzero(tie_x & ~tie_y), np.count_nonzero(~tie_x & tie_y),
                np.count_nonzero(tie_x & tie_y))
    return out


def kendall_from_counts(counts, m: int) -> float | None:
    """``scipy.stats.kendalltau(x, y).statistic`` (tau-b) from the integer pair counts of ``m`` items, in scipy's own order of
    operations; None when there are fewer than two items or a key is constant (scipy's NaN)."""
    m = int(m)
    if m < 2:
        return None
    _, discordant, tied_x, tied_y, tied_both = (int(v) for v in counts)
    total = m * (m - 1) // 2
    xtie, ytie = tied_x + tied_both, tied_y + tied_both  # the joint ties count on both sides
    if xtie == total or ytie == total:
        return None
    concordant_minus_discordant = total - xtie - ytie + tied_both - 2 * discordant
    tau = np.int64(concordant_minus_discordant) / np.sqrt(np.int64(total - xtie)) / np.sqrt(np.int64(total - ytie))
    return float(np.minimum(1.0, max(-1.0, tau)))


def spearman(x, y) -> float | None:
    """``scipy.stats.spearmanr`` of the two rank columns, as the reference takes it (:27-40): None below two items and for scipy's NaN."""
    from scipy.stats import spearmanr

    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if len(x) < 2:
        return None
    value = float(spearmanr(x, y).statistic)
    return None if np.isnan(value) else value


# ---- the membership ----
def _rank_column(series, name: str) -> np.ndarray:
    """A rank column (Int64 with nulls, or float64 with NaN) -> int64 with ``AGREE_NO_RANK`` for null."""
    import pandas as pd

    null = series.isna().to_numpy()
    values = pd.to_numeric(series, errors="coerce").to_numpy(dtype=np.float64, na_value=np.nan)
    present = values[~null]
    if np.isnan(present).any() or (present != np.floor(present)).any() or (present < 1).any() or (present >= 2.0 ** 31).any():
        raise ValueError(f"candidate provenance: {name} must be a positive integer below 2^31 or null")
    out = np.full(len(values), AGREE_NO_RANK, dtype=np.int64)
    out[~null] = present.astype(np.int64)
    return out


def membership_from_frame(frame, strategy_ids) -> dict:
    """The membership of a run from the reference's frame and the table's strategy ids (table order): ``{"frame": the columns read,
    "win_rate_rank", "trueskill_rank": int32 [n] in table order (AGREE_NO_RANK for null), "population_win_rate_rank",
    "population_trueskill_rank": int64 per frame row, "family_hash"}``.  Refuses what the reference refuses."""
    missing = [c for c in MEMBERSHIP_COLUMNS if c not in frame.columns]
    if missing:
        raise ValueError(f"candidate provenance lacks the columns {missing}")
    frame = frame[list(MEMBERSHIP_COLUMNS)].reset_index(drop=True).copy()
    names = frame["strategy"].astype(str)
    if names.duplicated().any():
        raise ValueError("candidate provenance contains duplicate strategies")
    table = [str(int(v)) for v in strategy_ids]
    final = frame["final_family"].astype(bool).to_numpy()
    if set(names[final]) != set(table) or len(set(table)) != len(table):
        raise ValueError("H2H inference finalist support differs from candidate provenance")
    hashes = set(frame.loc[final, "family_hash"].astype(str))
    if len(hashes) != 1:
        raise ValueError("candidate provenance must contain one final family hash")
    win, ts = _rank_column(frame["win_rate_rank"], "win_rate_rank"), _rank_column(frame["trueskill_rank"], "trueskill_rank")
    row_of = {name: r for r, name in enumerate(names)}
    rows = np.array([row_of[name] for name in table], dtype=np.int64)
    return {"frame": frame, "win_rate_rank": win[rows].astype(np.int32), "trueskill_rank": ts[rows].astype(np.int32),
            "population_win_rate_rank": win, "population_trueskill_rank": ts, "family_hash": next(iter(hashes))}


def read_membership(path, strategy_ids) -> dict:
    """``membership_from_frame`` of the reference's ``candidate_family.parquet`` at ``path``."""
    import pandas as pd

    return membership_from_frame(pd.read_parquet(path), strategy_ids)


def scored_population(membership: dict) -> tuple[np.ndarray, np.ndarray]:
    """The keys of ``rank_agreement`` (:27-32): both ranks of every row scored by both methods that has both — the whole scored
    population, not only the finalists."""
    win, ts = membership["population_win_rate_rank"], membership["population_trueskill_rank"]
    keep = membership["frame"]["scored_by_both_methods"].astype(bool).to_numpy() & (win != AGREE_NO_RANK) & (ts != AGREE_NO_RANK)
    return win[keep].astype(np.int32), ts[keep].astype(np.int32)


# ---- the artifacts ----
def _names(strategy_ids, n: int) -> np.ndarray:
    ids = np.arange(n, dtype=np.int64) if strategy_ids is None else np.asarray(strategy_ids, dtype=np.int64).reshape(-1)
    if len(ids) != n:
        raise ValueError(f"strategy_ids must name the {n} rows of the table")
    return np.array([str(int(v)) for v in ids], dtype=object)


def _side(field: np.ndarray) -> np.ndarray:
    return np.array([None, "a", "b"], dtype=object)[field]


def _tri_state(left: np.ndarray, right: np.ndarray):
    """Equal where both sides are not none, None elsewhere; a column without a None is boolean, as ``pd.DataFrame(rows)`` makes it."""
    available = (left != 0) & (right != 0)
    if available.all():
        return left == right
    out = np.full(len(left), None, dtype=object)
    out[available] = (left == right)[available].tolist()
    return out


def pairs_frame(codes, classes, strategy_ids=None, family_hash: str = ""):
    """``_pair_agreement``'s table (:73-125) from every pair's code and decision class, in pair-id order."""
    import pandas as pd

    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    cls = np.asarray(classes, dtype=np.int64).reshape(-1)
    if len(codes) != len(cls):
        raise ValueError("one code and one class per pair")
    n = int(round((1 + (1 + 8 * len(codes)) ** 0.5) / 2))
    if pair_count(n) != len(codes) or n < 2:
        raise ValueError(f"{len(codes)} pairs are not every pair of a table")
    names = _names(strategy_ids, n)
    pid, i, j = pair_ids(n)
    h, w, t = codes & 3, (codes >> 2) & 3, (codes >> 4) & 3
    return pd.DataFrame({
        "family_hash": np.full(len(codes), str(family_hash), dtype=object),
        "pair_id": pid.astype(np.int64),
        "strategy_a": names[i], "strategy_b": names[j],
        "decision_class": np.asarray(DECISION_CLASSES, dtype=object)[cls],
        "h2h_direction": _side(h), "win_rate_preference": _side(w), "trueskill_preference": _side(t),
        "win_rate_trueskill_agree": _tri_state(w, t),
        "h2h_agrees_with_win_rate": _tri_state(h, w),
        "h2h_agrees_with_trueskill": _tri_state(h, t),
        "selection_conditioning": np.full(len(codes), SELECTION_CONDITIONING, dtype=object),
    })[list(PAIR_COLUMNS)]


def _set_overlap(left: set, right: set) -> dict:
    union, intersection = left | right, left & right
    return {"win_rate_count": len(left), "trueskill_count": len(right), "intersection_count": len(intersection), "union_count": len(union),
            "jaccard": (len(intersection) / len(union)) if union else None}


def _fraction(agree: int, available: int) -> float | None:
    return int(agree) / int(available) if int(available) else None


def summary(membership: dict, counts, concordance, root_stability: dict | None, execution_scope: str) -> dict[str, Any]:
    """``_summary``'s dictionary (:133-216).  ``counts``: the eleven pair counts; ``concordance``: the five counts of
    ``scored_population(membership)`` (None when it has fewer than two rows); ``root_stability``:
    ``rr_root_diagnostics.stability_summary`` of the run, None when the diagnostics were not run."""
    frame = membership["frame"]
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if len(counts) != AGREE_COUNTS:
        raise ValueError(f"counts must hold {AGREE_COUNTS} counts")
    names = frame["strategy"].astype(str)
    flag = {name: frame[name].astype(bool).to_numpy() for name in MEMBERSHIP_FLAGS}
    members = {name: set(names[flag[name]]) for name in MEMBERSHIP_FLAGS[2:6]}
    final = flag["final_family"]
    x, y = scored_population(membership)
    if len(x) >= 2 and concordance is None:
        raise ValueError(f"the scored population has {len(x)} rows: their concordance counts are required")
    return {
        "family_hash": membership["family_hash"],
        "execution_scope": execution_scope,
        "conditioning": CONDITIONING,
        "common_scored_population_count": int(flag["scored_by_both_methods"].sum()),
        "rank_agreement": {"spearman": spearman(x, y), "kendall": kendall_from_counts(concordance, len(x)) if len(x) >= 2 else None},
        "initial_contribution_overlap": _set_overlap(members["initial_win_rate_contribution"], members["initial_trueskill_contribution"]),
        "final_contribution_overlap": _set_overlap(members["final_win_rate_contribution"], members["final_trueskill_contribution"]),
        "admission_counts": {
            "final_family": int(final.sum()),
            "win_rate": int((final & flag["final_win_rate_contribution"]).sum()),
            "trueskill": int((final & flag["final_trueskill_contribution"]).sum()),
            "shared": int((final & flag["final_shared_contribution"]).sum()),
            "controls": int((final & flag["configured_control"]).sum()),
            "mandatory_diagnostics": int((final & flag["mandatory_diagnostic"]).sum()),
        },
        "selection_conditioned_h2h": {
            "unordered_pair_count": int(counts[0]),
            "directional_pair_count": int(counts[1]),
            "unresolved_pair_count": int(counts[2]),
            "unresolved_nonviable_pair_count": int(counts[3]),
            "equivalent_pair_count": int(counts[4]),
            "win_rate_trueskill_direction_agreement_fraction": _fraction(counts[6], counts[5]),
            "h2h_win_rate_direction_agreement_fraction": _fraction(counts[8], counts[7]),
            "h2h_trueskill_direction_agreement_fraction": _fraction(counts[10], counts[9]),
        },
        "root_specific_h2h_stability": root_stability,
    }
