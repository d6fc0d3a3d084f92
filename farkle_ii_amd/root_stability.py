"""The two-root stability stage's bootstrap families from the batch matrices of two roots.

The reference (``src/farkle/analysis/root_stability.py``) picks up the ``performance_batch_matrix.npy`` of every (root, player count)
cell (``_matrix_cell`` :170-224), estimates every scope (``_scope_estimates`` :995-1054 -> ``_estimate_matrix_cells`` :348-498,
``_estimate_across_k`` :516-593), compares the roots (``_discrepancies`` :1099-1198) and runs two joint batch bootstraps over the
2 x n_k matrices: ``_RootTopNRangeWriter`` (:816-906, reduced by ``_root_bootstrap_top_n_inclusion`` :909-992) and
``_JointDiscrepancyRangeWriter`` (:1201-1311, reduced by ``_joint_discrepancy_bootstrap`` :1314-1426).  Both families draw the same
coordinate streams (``RandomPurpose.ROOT_STABILITY_BOOTSTRAP``) and do the same integer products, so one device pass serves both:
``Engine.root_stability_bootstrap`` (``fk_root_stability_bootstrap``, csrc/fk_root_stability.h) reproduces them bit for bit.

This module holds what stays on the host: loading and checking the cells (``load_cells``), the projection to eligible batches
(``project_cells``), the estimate chain in NumPy with the reference's expressions (``scope_estimates``, ``discrepancies``), the
drivers and seams (``run_root_bootstrap``, ``write_top_n_range``, ``write_joint_discrepancy_range``), the three frames
(``root_stability_tables``) and a NumPy HOST STATEMENT of the device's work (``host_root_bootstrap``: the real
``numpy.random.Generator(PCG64DXSM)`` behind ``random.coordinate_rng``), which is the oracle of the tests and the engine behind their
stub.

The stage's other eight frames (``build_two_root_stability`` :1761-1792: by-k and across-k root combination,
``_rank_and_selection_stability`` :634-748, ``_matched_count_convergence`` :1429-1513, ``_half_drift`` :1516-1628) repeat the estimate
chain over row windows of the cells.  ``Engine.root_window_estimates`` (``fk_root_window_estimates``, csrc/fk_root_windows.h) returns
the chain's sums for every window of the stage in one call; ``stage_windows`` lists the windows, ``window_pairwise_begin`` holds the
reference's column-chunk rule (which decides the summation order of a column), ``estimate_windows`` is the entry's NumPy host statement
and ``diagnostic_tables`` builds the frames.  ``estimate_scope`` stays as the one-chunk statement of the chain.

``across_k_estimates`` uses the reference's own ``np.dot``, whose bits depend on the BLAS kernel of the machine (fused multiply-adds):
it gives what the reference gives on the same machine, and nothing else can be promised for these two columns.  The device never sees
them computed: ``observed_across`` / ``expected_across`` are inputs of the entry.
"""
from __future__ import annotations

from dataclasses import dataclass
from math import sqrt
from pathlib import Path
from typing import Mapping, Sequence

import numpy as np

from .performance_bootstrap import BatchMatrix
from .random import RandomPurpose, coordinate_rng

ROOT_BOOTSTRAP_RANGE_SIZE = 50  # _ROOT_BOOTSTRAP_RANGE_SIZE :73
SCOPE_COMBINED = "combined_roots"


# ---- cells ---------------------------------------------------------------------------------------------------------------------
@dataclass
class RootCells:
    """The 2 x n_k batch matrices, checked: ``matrices[(root, k)]``, all with the strategy columns ``strategies``."""

    roots: tuple
    required_k: tuple
    strategies: np.ndarray  # int64 [S] ascending
    matrices: dict

    def in_order(self) -> list:
        return [self.matrices[(root, k)] for root in self.roots for k in self.required_k]


def check_roots(roots: Sequence[int]) -> tuple:
    """Exactly two different roots, ascending (``build_two_root_stability`` :1718-1720)."""
    found = tuple(sorted({int(r) for r in roots}))
    if len(found) != 2 or len(list(roots)) != 2:
        raise ValueError(f"two-root stability requires exactly two roots, found {tuple(int(r) for r in roots)}")
    return found


def check_cells(matrices: Mapping, roots: Sequence[int], required_k: Sequence[int], strategies: Sequence[int] | None = None) -> RootCells:
    """``matrices``: ``{(root, k): BatchMatrix}``.  Every root/k cell present (:1722-1729), each matrix of its cell's root (:218-222), all
    with identical strategy columns (:392-393, :835-838), which equal ``strategies`` when given."""
    pair = check_roots(roots)
    required = tuple(sorted(int(k) for k in required_k))
    if not required:
        raise ValueError("two-root stability requires at least one player count")
    expected = {(root, k) for root in pair for k in required}
    observed = {(int(root), int(k)) for root, k in matrices}
    if observed != expected:
        raise ValueError(f"two-root inputs must cover every root/k cell; missing={sorted(expected - observed)}, "
                         f"extra={sorted(observed - expected)}")
    ids = None if strategies is None else np.asarray(strategies, dtype=np.int64)
    for root in pair:
        for k in required:
            m = matrices[(root, k)]
            if int(m.root_seed) != root:
                raise ValueError(f"the {k}p batch matrix of root {root} has root support [{int(m.root_seed)}], expected [{root}]")
            if int(m.k) != k:
                raise ValueError(f"the batch matrix of cell (root {root}, {k}p) was loaded for {int(m.k)} players")
            if ids is None:
                ids = m.strategies.astype(np.int64)
            if not np.array_equal(m.strategies.astype(np.int64), ids):
                raise ValueError(f"root stability strategy support differs across matrices: cell (root {root}, {k}p)")
    return RootCells(pair, required, ids, {key: matrices[key] for key in sorted(expected)})


def load_cells(matrix_paths: Sequence, roots: Sequence[int], required_k: Sequence[int], strategies: Sequence[int] | None = None) -> RootCells:
    """``matrix_paths``: one canonical batch matrix per cell in (root, k) order, as the reference's range writers take them."""
    cells = [(int(root), int(k)) for root in roots for k in required_k]
    if len(list(matrix_paths)) != len(cells):
        raise ValueError(f"{len(cells)} batch matrices are required, one per root/k cell; got {len(list(matrix_paths))}")
    matrices = {}
    for (root, k), path in zip(cells, matrix_paths):
        if not Path(path).exists():
            raise ValueError(f"two-root inputs must cover every root/k cell; missing={[(root, k)]}: {path} does not exist")
        matrices[(root, k)] = BatchMatrix.load(path, k)
    return check_cells(matrices, roots, required_k, strategies)


@dataclass
class CellProjection:
    """What the samplers see (:840-850, :1231-1241): per cell, in (root, k) order, the wins / exposures of the eligible batches."""

    roots: tuple
    required_k: tuple
    strategies: np.ndarray
    wins: list       # per cell: int64 [B][S]
    exposures: list
    eligible: list   # per cell: positions of the eligible batches in the matrix


def project_cells(cells: RootCells) -> CellProjection:
    wins, exposures, eligible = [], [], []
    for m in cells.in_order():
        rows = np.flatnonzero(np.all(m.exposures > 0, axis=1))
        if not rows.size:
            raise ValueError("root bootstrap has no positive-exposure batch vectors")
        wins.append(np.ascontiguousarray(m.wins[rows]))
        exposures.append(np.ascontiguousarray(m.exposures[rows]))
        eligible.append(rows)
    return CellProjection(cells.roots, cells.required_k, cells.strategies, wins, exposures, eligible)


# ---- the estimate chain ----------------------------------------------------------------------------------------------------------
def k_weights(method: str, declared: Mapping | None, required_k: Sequence[int]) -> list:
    """``_k_weights`` (:501-513) as a list in the order of ``required_k``."""
    required = [int(k) for k in required_k]
    if method == "equal-k":
        return [1.0 / len(required)] * len(required)
    if declared is None or {int(k) for k in declared} != set(required):
        raise ValueError("declared k weights must cover complete configured support")
    weights = {int(k): float(v) for k, v in declared.items()}
    if abs(sum(weights.values()) - 1.0) > 1e-12:
        raise ValueError("declared k weights must sum to one")
    return [weights[k] for k in required]


def method_name(weights: Sequence[float]) -> str:
    """``cfg_method_name`` (:596-602)."""
    equal = 1.0 / len(weights)
    return "equal_k_mean" if all(abs(w - equal) <= 1e-15 for w in weights) else "declared_k_weighted_mean"


def threshold_position(effect: float, practical_delta: float) -> str:
    """``_practical_threshold_position`` (:240-247)."""
    if effect >= practical_delta:
        return "above_positive_threshold"
    if effect <= -practical_delta:
        return "below_negative_threshold"
    return "between_thresholds"


def estimate_scope(matrices: Sequence[BatchMatrix], k: int, practical_delta: float) -> dict:
    """``_estimate_matrix_cells`` (:348-498) for one scope (one root's matrix, or both for ``combined_roots``): ``chance_delta``,
    ``batch_mcse`` (NaN with fewer than two positive batches) and ``practical_threshold_position`` per strategy."""
    S = len(matrices[0].strategies)
    wins, exposures, positive_batches = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    sum_w2, sum_we, sum_e2 = np.zeros(S, np.float64), np.zeros(S, np.float64), np.zeros(S, np.float64)
    for m in matrices:
        wins += np.asarray(m.wins).sum(axis=0, dtype=np.int64)
        exposures += np.asarray(m.exposures).sum(axis=0, dtype=np.int64)
        batch_wins = np.asarray(m.wins, dtype=np.float64)
        batch_exposures = np.asarray(m.exposures, dtype=np.float64)
        positive = batch_exposures > 0
        positive_batches += positive.sum(axis=0, dtype=np.int64)
        batch_wins = np.where(positive, batch_wins, 0.0)
        batch_exposures = np.where(positive, batch_exposures, 0.0)
        sum_w2 += np.sum(batch_wins * batch_wins, axis=0)
        sum_we += np.sum(batch_wins * batch_exposures, axis=0)
        sum_e2 += np.sum(batch_exposures * batch_exposures, axis=0)
    if np.any(exposures <= 0):
        raise ValueError("root stability scope contains a strategy without positive exposure")
    rates = wins / exposures
    mcse = np.full(S, np.nan, dtype=np.float64)
    eligible = positive_batches >= 2
    if np.any(eligible):
        residual_squares = sum_w2[eligible] - 2.0 * rates[eligible] * sum_we[eligible] + rates[eligible] ** 2 * sum_e2[eligible]
        variance = positive_batches[eligible] / (positive_batches[eligible] - 1.0)
        variance *= np.maximum(residual_squares, 0.0)
        mcse[eligible] = np.sqrt(variance) / exposures[eligible]
    effects = rates - 1.0 / k
    return {"chance_delta": effects, "batch_mcse": mcse,
            "practical_threshold_position": [threshold_position(float(e), practical_delta) for e in effects]}


# ---- row windows: the sums of the estimate chain over any rows of any cell -------------------------------------------------------
WINDOW_BYTES_PER_CELL = 7 * 8 + 1  # bytes_per_cell of ``_estimate_matrix_cells`` (:403)
DEFAULT_STAGE_BATCH_BYTES = 16 << 20  # resources.stage_batch_bytes["performance"] when nothing is configured
WINDOW_TOTALS = ("wins", "exposures", "completed", "safety", "losses", "positive_batches")
WINDOW_SUMS = ("sum_w2", "sum_we", "sum_e2")


def window_chunk(S: int, rows: int, max_bytes: int) -> int:
    """The column chunk of ``_estimate_matrix_cells`` (:404-410) for a window of ``rows`` rows: the one place the formula is written."""
    return max(1, min(int(S), int(max_bytes) // max(1, int(rows) * WINDOW_BYTES_PER_CELL)))


def window_pairwise_begin(S: int, rows: int, max_bytes: int) -> int:
    """The first column of a window that falls into a chunk of width 1, ``S`` when none does.  ``np.sum(x, axis=0)`` over such a
    chunk sums a vector (NumPy's pairwise order); over a wider one it adds row by row.  Chunks of width 1 arise when ``S == 1``,
    when the chunk is 1 (every column) and for the last column when ``S % chunk == 1``."""
    chunk = window_chunk(S, rows, max_bytes)
    if chunk == 1:
        return 0
    return int(S) - 1 if int(S) % chunk == 1 else int(S)


def stage_window(cell: int, row_begin: int, row_end: int, S: int, max_bytes: int) -> tuple:
    """One row of ``Engine.root_window_estimates``'s window list: ``(cell, row_begin, row_end, pairwise_begin)``."""
    return (int(cell), int(row_begin), int(row_end), window_pairwise_begin(S, int(row_end) - int(row_begin), max_bytes))


def estimate_windows(wins: Sequence, exposures: Sequence, completed: Sequence, safety: Sequence, windows) -> dict:
    """``Engine.root_window_estimates`` in NumPy: the same arguments, the same result.  Per window the expressions of
    ``_estimate_matrix_cells`` (:411-433) over rows ``[row_begin, row_end)`` of the cell, the columns cut as the window's
    ``pairwise_begin`` says: ``[0, pairwise_begin)`` summed as a chunk of two or more columns, every later column as a chunk of its
    own.  (A ``pairwise_begin`` of 1, which the chunk rule never gives, widens its lone column by a copy of itself: the entry defines
    the row-by-row order for it.)  int64 ``[n][S]`` totals (``WINDOW_TOTALS``) and float64 ``[n][S]`` sums (``WINDOW_SUMS``)."""
    kinds = [[np.asarray(m, dtype=np.int64) for m in group] for group in (wins, exposures, completed, safety)]
    n_cells = len(kinds[0])
    if not n_cells or any(len(group) != n_cells for group in kinds):
        raise ValueError("one wins / exposures / completed / safety matrix per cell")
    S = int(kinds[0][0].shape[1]) if kinds[0][0].ndim == 2 else -1
    for cell in range(n_cells):
        w, e, c, f = (group[cell] for group in kinds)
        if any(m.ndim != 2 or m.shape != w.shape or m.shape[1] != S for m in (w, e, c, f)) or S < 1 or not len(w):
            raise ValueError("every matrix is [batches][S] with one S and at least one batch, the four of a cell of one shape")
        if min(int(m.min()) for m in (w, e, c, f)) < 0:
            raise ValueError(f"cell {cell}: a negative count")
        if np.any(w > c):
            raise ValueError(f"cell {cell}: wins > completed: impossible win/exposure counts")
        if np.any(c + f != e):
            raise ValueError(f"cell {cell}: exposures != completed + safety: attempted exposure conservation")
        high, low = (e >> 31).sum(axis=0, dtype=np.int64).tolist(), (e & (2 ** 31 - 1)).sum(axis=0, dtype=np.int64).tolist()  # exact halves
        if any((h << 31) + l > 2 ** 62 for h, l in zip(high, low)):
            raise ValueError(f"cell {cell}: the exposure total of a column passes 2^62")
    windows = np.asarray(windows, dtype=np.int64)
    if windows.ndim != 2 or windows.shape[1] != 4 or not len(windows):
        raise ValueError("windows is [n][4] with n >= 1: cell, row_begin, row_end, pairwise_begin")
    out = {name: np.zeros((len(windows), S), dtype=np.int64) for name in WINDOW_TOTALS}
    out.update({name: np.zeros((len(windows), S), dtype=np.float64) for name in WINDOW_SUMS})
    for i, (cell, start, stop, pairwise_begin) in enumerate(windows.tolist()):
        if not 0 <= cell < n_cells:
            raise ValueError(f"window {i}: cell {cell} of {n_cells}")
        if start < 0 or stop <= start or stop > len(kinds[0][cell]):
            raise ValueError(f"window {i}: root stability matrix slice is empty or invalid")
        if not 0 <= pairwise_begin <= S:
            raise ValueError(f"window {i}: pairwise_begin = {pairwise_begin} outside [0, {S}]")
        chunks = ([(0, pairwise_begin)] if pairwise_begin else []) + [(s, s + 1) for s in range(pairwise_begin, S)]
        for column_start, column_stop in chunks:
            columns = slice(column_start, column_stop)
            widen = column_start == 0 and pairwise_begin == 1  # the lone row-by-row column
            keep = slice(0, 1) if widen else slice(None)
            for name, group in zip(WINDOW_TOTALS[:4], kinds):
                out[name][i, columns] += np.asarray(group[cell][start:stop, columns]).sum(axis=0, dtype=np.int64)
            batch_wins = np.asarray(kinds[0][cell][start:stop, columns], dtype=np.float64)
            batch_exposures = np.asarray(kinds[1][cell][start:stop, columns], dtype=np.float64)
            if widen:
                batch_wins, batch_exposures = np.repeat(batch_wins, 2, axis=1), np.repeat(batch_exposures, 2, axis=1)
            positive = batch_exposures > 0
            out["positive_batches"][i, columns] += positive.sum(axis=0, dtype=np.int64)[keep]
            batch_wins = np.where(positive, batch_wins, 0.0)
            batch_exposures = np.where(positive, batch_exposures, 0.0)
            out["sum_w2"][i, columns] += np.sum(batch_wins * batch_wins, axis=0)[keep]
            out["sum_we"][i, columns] += np.sum(batch_wins * batch_exposures, axis=0)[keep]
            out["sum_e2"][i, columns] += np.sum(batch_exposures * batch_exposures, axis=0)[keep]
        out["losses"][i] = out["exposures"][i] - out["wins"][i]
        if np.any(out["exposures"][i] <= 0):
            raise ValueError(f"window {i}: root stability scope contains a strategy without positive exposure")
    return out


class HostEngine:
    """``estimate_windows`` behind the engine's method name: the engine of the host path and of the tests' stub."""

    def root_window_estimates(self, wins, exposures, completed, safety, windows) -> dict:
        return estimate_windows(wins, exposures, completed, safety, windows)

    def rank_concordance(self, x, y) -> np.ndarray:
        from .structure_agreement import concordance_counts

        return concordance_counts(x, y)


def scope_from_windows(sums: Mapping, windows: Sequence[int], k: int, practical_delta: float) -> dict:
    """``estimate_scope`` from window sums: the windows at positions ``windows`` of ``sums`` (``estimate_windows`` or the engine's),
    one per matrix of the scope, added in the reference's order — ``0 + a`` for a root, ``0 + a + b`` for ``combined_roots`` (:413-433
    inside the loop over the paths) — then the expressions of :442-462."""
    S = np.asarray(sums["wins"]).shape[1]
    wins, exposures, positive_batches = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    sum_w2, sum_we, sum_e2 = np.zeros(S, np.float64), np.zeros(S, np.float64), np.zeros(S, np.float64)
    for i in windows:
        wins += sums["wins"][i]
        exposures += sums["exposures"][i]
        positive_batches += sums["positive_batches"][i]
        sum_w2 += sums["sum_w2"][i]
        sum_we += sums["sum_we"][i]
        sum_e2 += sums["sum_e2"][i]
    if np.any(exposures <= 0):
        raise ValueError("root stability scope contains a strategy without positive exposure")
    rates = wins / exposures
    mcse = np.full(S, np.nan, dtype=np.float64)
    eligible = positive_batches >= 2
    if np.any(eligible):
        residual_squares = sum_w2[eligible] - 2.0 * rates[eligible] * sum_we[eligible] + rates[eligible] ** 2 * sum_e2[eligible]
        variance = positive_batches[eligible] / (positive_batches[eligible] - 1.0)
        variance *= np.maximum(residual_squares, 0.0)
        mcse[eligible] = np.sqrt(variance) / exposures[eligible]
    effects = rates - 1.0 / k
    return {"chance_delta": effects, "batch_mcse": mcse,
            "practical_threshold_position": [threshold_position(float(e), practical_delta) for e in effects]}


def stage_windows(batch_counts: Sequence[int], S: int, max_bytes: int, matched_count_fractions: Sequence[float]) -> tuple:
    """The window list of the whole stage, built once: per cell (in ``RootCells.in_order``) the full matrix (``_scope_estimates``),
    the matched-count prefixes (``_matched_count_convergence`` :1438-1452: ``min(minimum, max(1, ceil(minimum * fraction)))`` rows of
    every cell) and both halves (``_half_drift`` :1540-1544; a cell with fewer than two batches is refused there).  Duplicates are
    dropped.  -> ``(windows int64 [n][4], index)``, ``index[(cell, row_begin, row_end)]`` the window's position."""
    from math import ceil

    counts = [int(b) for b in batch_counts]
    minimum = min(counts)
    matched = [min(minimum, max(1, ceil(minimum * float(fraction)))) for fraction in matched_count_fractions]
    rows, index = [], {}
    for cell, count in enumerate(counts):
        if count < 2:
            raise ValueError(f"cell {cell} needs at least two batches for drift")
        midpoint = count // 2
        for start, stop in [(0, count)] + [(0, m) for m in matched] + [(0, midpoint), (midpoint, count)]:
            if (cell, start, stop) not in index:
                index[(cell, start, stop)] = len(rows)
                rows.append(stage_window(cell, start, stop, S, max_bytes))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4), index


def across_k_estimates(values: np.ndarray, mcse: np.ndarray, weights: Sequence[float]) -> tuple:
    """``_estimate_across_k`` (:558-563): ``values`` / ``mcse`` are ``[n_k][S]``; per strategy ``float(np.dot(weights, values))`` and
    ``sqrt(np.dot(weights * weights, mcse ** 2))`` — the reference's own expression (see the module docstring)."""
    values, mcse = np.asarray(values, dtype=np.float64), np.asarray(mcse, dtype=np.float64)
    S = values.shape[1]
    score, error = np.empty(S, np.float64), np.empty(S, np.float64)
    weight_array = np.asarray(list(weights), dtype=float)
    for s in range(S):
        column = np.asarray([float(v) for v in values[:, s]], dtype=float)
        variances = np.asarray([float(v) ** 2 for v in mcse[:, s]], dtype=float)
        score[s] = float(np.dot(weight_array, column))
        error[s] = float(sqrt(np.dot(weight_array * weight_array, variances)))
    return score, error


@dataclass
class ScopeEstimates:
    scopes: tuple     # ("root_<a>", "root_<b>", "combined_roots")
    by_k: dict        # {k: {scope: estimate_scope(...)}}
    across: dict      # {scope: {"across_k_score", "across_k_mcse", "practical_threshold_position"}}


def scope_estimates(cells: RootCells, weights: Sequence[float], practical_delta_by_k: Mapping | None, delta_across_k: float | None,
                    across_k: Mapping | None = None) -> ScopeEstimates:
    """``_scope_estimates`` (:995-1054).  ``across_k``: ``{scope: (across_k_score, across_k_mcse)}`` replaces the ``np.dot`` columns
    (the tests feed a fixture's recorded columns, which hold only on the machine that wrote them)."""
    if practical_delta_by_k is None:
        raise ValueError("screening.practical_delta_by_k is required")
    if delta_across_k is None:
        raise ValueError("screening.delta_across_k is required")
    practical = {int(k): float(v) for k, v in practical_delta_by_k.items()}
    missing = [k for k in cells.required_k if k not in practical]
    if missing:
        raise ValueError(f"screening.practical_delta_by_k is required for every player count; missing {missing}")
    a, b = cells.roots
    scopes = (f"root_{a}", f"root_{b}", SCOPE_COMBINED)
    by_k = {}
    for k in cells.required_k:
        by_k[k] = {scopes[0]: estimate_scope([cells.matrices[(a, k)]], k, practical[k]),
                   scopes[1]: estimate_scope([cells.matrices[(b, k)]], k, practical[k]),
                   scopes[2]: estimate_scope([cells.matrices[(a, k)], cells.matrices[(b, k)]], k, practical[k])}
    across = {}
    for scope in scopes:
        if across_k is not None:
            score, error = (np.asarray(v, dtype=np.float64) for v in across_k[scope])
        else:
            score, error = across_k_estimates(np.stack([by_k[k][scope]["chance_delta"] for k in cells.required_k]),
                                              np.stack([by_k[k][scope]["batch_mcse"] for k in cells.required_k]), weights)
        across[scope] = {"across_k_score": score, "across_k_mcse": error,
                         "practical_threshold_position": [threshold_position(float(v), float(delta_across_k)) for v in score]}
    return ScopeEstimates(scopes, by_k, across)


def safe_standardized(raw_difference: float, expected_mcse: float) -> float | None:
    """``_safe_standardized`` (:1057-1069)."""
    if expected_mcse is None or not np.isfinite(expected_mcse):
        return None
    if expected_mcse > 0.0:
        return raw_difference / expected_mcse
    if raw_difference == 0.0:
        return 0.0
    return float(np.copysign(np.inf, raw_difference))


DISCREPANCY_COLUMNS = ("estimand_scope", "k", "strategy", "root_a", "root_b", "root_a_estimate", "root_b_estimate", "combined_estimate",
                       "raw_difference", "expected_mcse", "standardized_discrepancy", "stability_threshold", "threshold_fraction",
                       "root_a_practical_threshold_position", "root_b_practical_threshold_position",
                       "combined_practical_threshold_position", "practical_threshold_position_changed")


def discrepancies(estimates: ScopeEstimates, cells: RootCells, stability_threshold: float) -> dict:
    """``_discrepancies`` (:1099-1198): the 17 columns as lists, by-k rows (player counts ascending) then across-k rows, strategies
    ascending within each.  ``k`` and ``standardized_discrepancy`` hold ``None`` where the reference does."""
    root_a, root_b = cells.roots
    scope_a, scope_b, scope_c = estimates.scopes
    out = {name: [] for name in DISCREPANCY_COLUMNS}
    threshold = stability_threshold

    def rows(scope_name, k, a, b, combined, value, error):
        for s, strategy in enumerate(cells.strategies.tolist()):
            estimate_a, estimate_b = float(a[value][s]), float(b[value][s])
            raw = estimate_a - estimate_b
            expected = sqrt(float(a[error][s]) ** 2 + float(b[error][s]) ** 2)
            positions = [scope["practical_threshold_position"][s] for scope in (a, b, combined)]
            for name, item in zip(DISCREPANCY_COLUMNS, (
                    scope_name, k, int(strategy), root_a, root_b, estimate_a, estimate_b, float(combined[value][s]), raw, expected,
                    safe_standardized(raw, expected), threshold, abs(raw) / threshold, *positions, positions[0] != positions[1])):
                out[name].append(item)

    for k in cells.required_k:
        rows("by_k", k, estimates.by_k[k][scope_a], estimates.by_k[k][scope_b], estimates.by_k[k][scope_c], "chance_delta", "batch_mcse")
    rows("across_k", None, estimates.across[scope_a], estimates.across[scope_b], estimates.across[scope_c], "across_k_score", "across_k_mcse")
    return out


@dataclass
class JointInputs:
    """What ``_joint_discrepancy_bootstrap`` hands its writer (:1337-1344): ``observed`` / ``expected`` ``[n_k][S]`` and the across-k
    pair ``[S]``, from the discrepancy rows' ``raw_difference`` / ``expected_mcse``."""

    observed: np.ndarray
    expected: np.ndarray
    observed_across: np.ndarray
    expected_across: np.ndarray


def joint_inputs(frame: Mapping, n_k: int, S: int) -> JointInputs:
    raw = np.asarray([float("nan") if v is None else v for v in frame["raw_difference"]], dtype=np.float64)
    expected = np.asarray([float("nan") if v is None else v for v in frame["expected_mcse"]], dtype=np.float64)
    if raw.shape != ((n_k + 1) * S,):
        raise ValueError("the discrepancy frame does not hold one row per (player count or across-k, strategy)")
    return JointInputs(raw[:n_k * S].reshape(n_k, S), expected[:n_k * S].reshape(n_k, S), raw[n_k * S:], expected[n_k * S:])


# ---- the host statement -------------------------------------------------------------------------------------------------------
def resample_counts(root_seed: int, k: int, replicate: int, n_batches: int) -> np.ndarray:
    """The multiplicities of one (replicate, root, player count) stream (:864-873, :1251-1260), by numpy's own generator."""
    rng = coordinate_rng(RandomPurpose.ROOT_STABILITY_BOOTSTRAP, root_seed=int(root_seed), k=int(k), replicate_index=int(replicate))
    selected = rng.integers(0, n_batches, size=n_batches)
    return np.bincount(selected, minlength=n_batches).astype(np.int64, copy=False)


def _checked_arguments(roots, ks, wins, exposures, weights, top_n, observed, expected, observed_across, expected_across):
    roots = [int(r) for r in roots]
    if len(roots) != 2 or not roots[0] < roots[1]:
        raise ValueError("two roots (a, b) with a < b are required")
    ks = [int(k) for k in ks]
    n_k = len(ks)
    weights = [float(w) for w in weights]
    if not n_k or len(weights) != n_k or len(wins) != 2 * n_k or len(exposures) != 2 * n_k:
        raise ValueError("one weight per player count and one wins / exposures matrix per (root, player count) cell are required")
    if not all(np.isfinite(weights)):
        raise ValueError("a weight is not finite")
    W = [np.asarray(m, dtype=np.int64) for m in wins]
    E = [np.asarray(m, dtype=np.int64) for m in exposures]
    S = int(W[0].shape[1]) if W[0].ndim == 2 else -1
    for w, e in zip(W, E):
        if w.ndim != 2 or w.shape != e.shape or w.shape[1] != S or S < 1 or not len(w):
            raise ValueError("every matrix is [batches][S] with one S and at least one batch")
        if np.any(w < 0) or np.any(e < 0):
            raise ValueError("negative count")
        if max(int(w.max()), int(e.max())) >= 2 ** 63 // len(w):
            raise ValueError("a count whose resampled total can pass 2**63")
    if not 0 <= int(top_n) <= S:
        raise ValueError("top_n must be in [0, S]")
    group = [observed, expected, observed_across, expected_across]
    given = sum(v is not None for v in group)
    if given not in (0, 4):
        raise ValueError("observed / expected by k and across k come as a group of four")
    joint = None
    if given:
        joint = JointInputs(np.ascontiguousarray(observed, dtype=np.float64).reshape(n_k, S), np.ascontiguousarray(expected, dtype=np.float64).reshape(n_k, S),
                            np.ascontiguousarray(observed_across, dtype=np.float64).reshape(S), np.ascontiguousarray(expected_across, dtype=np.float64).reshape(S))
        if not (np.all(np.isfinite(joint.observed)) and np.all(np.isfinite(joint.observed_across))):
            raise ValueError("observed is not finite")
    return roots, ks, weights, W, E, S, joint


def host_root_bootstrap(roots, ks, wins, exposures, weights, replicate_begin: int, replicate_end: int, top_n: int, observed=None,
                        expected=None, observed_across=None, expected_across=None, want_membership: bool = False) -> dict:
    """``Engine.root_stability_bootstrap`` in NumPy: the same arguments, the same result.  Per replicate the rates of every cell
    (:1246-1287), the top-N membership of both roots (:859-902) and the joint maximum (:1288-1307)."""
    roots, ks, weights, W, E, S, joint = _checked_arguments(roots, ks, wins, exposures, weights, top_n, observed, expected, observed_across,
                                                            expected_across)
    n_k = len(ks)
    R = max(int(replicate_end) - int(replicate_begin), 0)
    if int(replicate_begin) < 0 or int(replicate_end) < int(replicate_begin):
        raise ValueError("bad replicate range")
    columns = np.arange(S, dtype=np.int64)
    top_counts = np.zeros((2, S), dtype=np.int64)
    membership = np.zeros((R, 2, S), dtype=np.uint8)
    maxima = np.zeros(R, dtype=np.float64)
    for row, replicate in enumerate(range(int(replicate_begin), int(replicate_end))):
        rates = {}
        for root_index, root in enumerate(roots):
            for ki, k in enumerate(ks):
                cell = root_index * n_k + ki
                counts = resample_counts(root, k, replicate, len(W[cell]))
                total_wins = counts @ W[cell]  # exact int64
                total_exposures = counts @ E[cell]
                if np.any(total_exposures <= 0):
                    raise ValueError("root bootstrap produced zero complete-support exposure")
                rates[(root_index, ki)] = total_wins / total_exposures - 1.0 / k
        for root_index in range(2):
            scores = np.zeros(S, dtype=np.float64)
            for ki, weight in enumerate(weights):
                scores += weight * rates[(root_index, ki)]
            order = np.lexsort((columns, -scores))
            membership[row, root_index, order[:int(top_n)]] = 1
        if joint is not None:
            standardized = []
            state = np.seterr(over="ignore")  # (a denormal expected: the quotient is +inf, as on the device)
            for ki in range(n_k):
                valid = joint.expected[ki] > 0.0
                centered = rates[(0, ki)] - rates[(1, ki)] - joint.observed[ki]
                standardized.append(np.abs(centered[valid] / joint.expected[ki][valid]))
            across = sum(weight * (rates[(0, ki)] - rates[(1, ki)]) for ki, weight in enumerate(weights))
            valid_across = joint.expected_across > 0.0
            standardized.append(np.abs((across - joint.observed_across)[valid_across] / joint.expected_across[valid_across]))
            np.seterr(**state)
            maxima[row] = max((float(part.max()) for part in standardized if part.size), default=0.0)
    top_counts += membership.sum(axis=0, dtype=np.int64)
    return {"top_counts": top_counts, "maxima": maxima if joint is not None else None, "membership": membership if want_membership else None}


# ---- drivers, seams and frames -----------------------------------------------------------------------------------------------------
def run_root_bootstrap(engine, projection: CellProjection, weights: Sequence[float], replicates: int, top_n: int,
                       joint: JointInputs | None, range_size: int | None = None) -> tuple:
    """All replicates through ``engine.root_stability_bootstrap`` -> ``(top_counts [2][S], maxima [replicates] or None)``.
    ``range_size``: replicates per call (default all in one: the device blocks the range itself).  Counts add and maxima are per
    replicate, so any split gives the same bits."""
    S = len(projection.strategies)
    step = int(range_size) if range_size else max(int(replicates), 1)
    top_counts = np.zeros((2, S), dtype=np.int64)
    maxima = np.zeros(int(replicates), dtype=np.float64) if joint is not None else None
    extra = {} if joint is None else {"observed": joint.observed, "expected": joint.expected, "observed_across": joint.observed_across,
                                      "expected_across": joint.expected_across}
    for start in range(0, int(replicates), step):
        stop = min(start + step, int(replicates))
        res = engine.root_stability_bootstrap(projection.roots, projection.required_k, projection.wins, projection.exposures, weights, start,
                                              stop, top_n, **extra)
        top_counts += res["top_counts"]
        if joint is not None:
            maxima[start:stop] = res["maxima"]
    return top_counts, maxima


def write_top_n_range(engine, matrix_paths: Sequence, roots: Sequence[int], required_k: Sequence[int], strategies: Sequence[int],
                      weights: Sequence[float], top_n: int, start: int, stop: int, path) -> None:
    """What the reference's ``_RootTopNRangeWriter(matrix_paths, roots, required_k, strategies, weights, top_n, ...)`` writes for the
    unit ``(start, stop)``: a ``.npy`` of uint8 ``[stop - start][2][len(strategies)]`` top-N membership (:816-906), computed by
    ``engine.root_stability_bootstrap``.  A seam a reference maintainer binds."""
    projection = project_cells(load_cells(matrix_paths, roots, required_k, strategies))
    res = engine.root_stability_bootstrap(projection.roots, projection.required_k, projection.wins, projection.exposures,
                                          [float(w) for w in weights], int(start), int(stop), int(top_n), want_membership=True)
    out = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=(int(stop) - int(start), 2, len(projection.strategies)))
    out[:] = res["membership"]
    out.flush()
    del out


def write_joint_discrepancy_range(engine, matrix_paths: Sequence, roots: Sequence[int], required_k: Sequence[int], strategies: Sequence[int],
                                  weights: Sequence[float], observed_by_k: Sequence, observed_across: Sequence[float],
                                  expected_across: Sequence[float], start: int, stop: int, path) -> None:
    """What the reference's ``_JointDiscrepancyRangeWriter(matrix_paths, roots, required_k, strategies, weights, observed_by_k,
    observed_across, expected_across, ...)`` writes for the unit ``(start, stop)``: a ``.npy`` of ``<f8 [stop - start]`` maxima
    (:1201-1311).  ``observed_by_k``: ``(k, observed, expected)`` per player count, as the writer's field."""
    projection = project_cells(load_cells(matrix_paths, roots, required_k, strategies))
    by_k = {int(k): (np.asarray(o, dtype=np.float64), np.asarray(e, dtype=np.float64)) for k, o, e in observed_by_k}
    if sorted(by_k) != list(projection.required_k):
        raise ValueError("observed_by_k must cover every required player count")
    res = engine.root_stability_bootstrap(projection.roots, projection.required_k, projection.wins, projection.exposures,
                                          [float(w) for w in weights], int(start), int(stop), 0,
                                          observed=np.stack([by_k[k][0] for k in projection.required_k]),
                                          expected=np.stack([by_k[k][1] for k in projection.required_k]),
                                          observed_across=np.asarray(observed_across, dtype=np.float64),
                                          expected_across=np.asarray(expected_across, dtype=np.float64))
    out = np.lib.format.open_memmap(path, mode="w+", dtype=np.dtype("<f8"), shape=(int(stop) - int(start),))
    out[:] = res["maxima"]
    out.flush()
    del out


def top_n_inclusion_schema():
    import pyarrow as pa

    return pa.schema([("root_seed", pa.int64()), ("strategy", pa.int32()), ("required_k_count", pa.int64()), ("complete_support", pa.bool_()),
                      ("k_aggregation_method", pa.string()), ("bootstrap_replicates", pa.int64()), ("top_n_size", pa.int64()),
                      ("bootstrap_top_n_inclusion_frequency", pa.float64())])


def discrepancy_schema():
    import pyarrow as pa

    text = {"estimand_scope", "root_a_practical_threshold_position", "root_b_practical_threshold_position",
            "combined_practical_threshold_position"}
    fields = []
    for name in DISCREPANCY_COLUMNS:
        kind = (pa.string() if name in text else pa.int32() if name == "strategy" else pa.int64() if name in ("root_a", "root_b")
                else pa.bool_() if name == "practical_threshold_position_changed" else pa.float64())
        fields.append((name, kind))
    return pa.schema(fields + [("joint_max_abs_standardized_reference_quantile", pa.float64()), ("exceeds_joint_reference_quantile", pa.bool_()),
                               ("joint_bootstrap_exceedance_frequency", pa.float64())])


def joint_summary_schema():
    import pyarrow as pa

    return pa.schema([("root_a", pa.int64()), ("root_b", pa.int64()), ("bootstrap_replicates", pa.int64()),
                      ("joint_reference_upper_tail_fraction", pa.float64()), ("maximum_absolute_standardized_discrepancy", pa.float64()),
                      ("joint_max_abs_standardized_reference_quantile", pa.float64()), ("observed_max_exceeds_joint_reference_quantile", pa.bool_()),
                      ("estimands_exceeding_joint_reference_quantile", pa.int64()), ("interpretation", pa.string())])


def _nullable(values) -> "object":
    """A float column as pandas hands it to Arrow (``Table.from_pandas``): ``None`` and NaN become nulls."""
    import pyarrow as pa

    return pa.array(np.asarray([float("nan") if v is None else v for v in values], dtype=np.float64), type=pa.float64(), from_pandas=True)


def top_n_inclusion_table(top_counts: np.ndarray, cells_roots: Sequence[int], strategies: np.ndarray, n_k: int, weights: Sequence[float],
                          replicates: int, top_n: int):
    """The frame of ``_root_bootstrap_top_n_inclusion`` (:975-992): rows root-major, strategies ascending."""
    import pyarrow as pa

    S = len(strategies)
    counts = np.asarray(top_counts, dtype=np.int64).reshape(2, S)
    return pa.Table.from_pydict({
        "root_seed": np.repeat(np.asarray(cells_roots, dtype=np.int64), S), "strategy": np.tile(np.asarray(strategies), 2).astype(np.int32),
        "required_k_count": np.full(2 * S, n_k, np.int64), "complete_support": np.ones(2 * S, dtype=bool),
        "k_aggregation_method": [method_name(weights)] * (2 * S), "bootstrap_replicates": np.full(2 * S, int(replicates), np.int64),
        "top_n_size": np.full(2 * S, int(top_n), np.int64),
        "bootstrap_top_n_inclusion_frequency": (counts / int(replicates)).reshape(-1)}, schema=top_n_inclusion_schema())


def joint_tables(frame: Mapping, maxima: np.ndarray, roots: Sequence[int], replicates: int, alpha: float):
    """``_joint_discrepancy_bootstrap``'s reduction (:1393-1426): the discrepancy frame enriched with the three joint columns, and the
    one-row summary, as Arrow tables with the types ``_write_frame`` leaves."""
    import pyarrow as pa

    standardized = frame["standardized_discrepancy"]
    if all(v is None for v in standardized):
        raise ValueError("no discrepancy has a finite expected MCSE (every cell needs at least two positive-exposure batches in some "
                         "player count): there is no standardized discrepancy to calibrate, and the reference's reduction fails here too")
    maxima = np.asarray(maxima, dtype=np.float64)
    values = np.asarray([float("nan") if v is None else v for v in standardized], dtype=np.float64)
    quantile = float(np.quantile(maxima, 1.0 - alpha, method="higher"))
    with np.errstate(invalid="ignore"):
        exceeds = np.abs(values) > quantile
    frequency = [(1.0 + float(np.count_nonzero(maxima >= abs(v)))) / (replicates + 1.0) for v in values.tolist()]
    n = len(values)
    columns = {}
    for name in DISCREPANCY_COLUMNS:
        column = frame[name]
        if name in ("k", "root_a_estimate", "root_b_estimate", "combined_estimate", "raw_difference", "expected_mcse",
                    "standardized_discrepancy", "stability_threshold", "threshold_fraction"):
            columns[name] = _nullable(column)
        else:
            columns[name] = column
    columns["joint_max_abs_standardized_reference_quantile"] = np.full(n, quantile, np.float64)
    columns["exceeds_joint_reference_quantile"] = exceeds
    columns["joint_bootstrap_exceedance_frequency"] = np.asarray(frequency, dtype=np.float64)
    enriched = pa.Table.from_pydict(columns, schema=discrepancy_schema())
    finite = np.abs(values[np.isfinite(values)])
    observed_max = float(finite.max()) if finite.size else float("inf")
    summary = pa.Table.from_pydict({
        "root_a": [int(roots[0])], "root_b": [int(roots[1])], "bootstrap_replicates": [int(replicates)],
        "joint_reference_upper_tail_fraction": [float(alpha)], "maximum_absolute_standardized_discrepancy": [observed_max],
        "joint_max_abs_standardized_reference_quantile": [quantile], "observed_max_exceeds_joint_reference_quantile": [observed_max > quantile],
        "estimands_exceeding_joint_reference_quantile": [int(np.count_nonzero(exceeds))],
        "interpretation": ["reproducibility_diagnostic_not_root_random_effect"]}, schema=joint_summary_schema())
    return enriched, summary


def root_stability_tables(engine, cells: RootCells, replicates: int, candidate_contribution_size: int,
                          practical_delta_by_k: Mapping | None, delta_across_k: float | None, delta_seed_stability: float,
                          joint_discrepancy_alpha: float, k_aggregation_method: str = "equal-k", declared_k_weights: Mapping | None = None,
                          range_size: int | None = None, across_k: Mapping | None = None, estimates: ScopeEstimates | None = None) -> dict:
    """From the checked cells to the three frames ``root_bootstrap_top_n_inclusion``, ``root_discrepancies`` (enriched) and
    ``root_joint_discrepancy``: estimate chain, one ``engine.root_stability_bootstrap`` pass for both families, reductions.
    ``estimates``: the chain's estimates when the caller has them already (``diagnostic_tables``: from the window call)."""
    if int(replicates) < 1:
        raise ValueError("screening.bootstrap_replicates must be positive")
    weights = k_weights(k_aggregation_method, declared_k_weights, cells.required_k)
    if estimates is None:
        estimates = scope_estimates(cells, weights, practical_delta_by_k, delta_across_k, across_k=across_k)
    frame = discrepancies(estimates, cells, float(delta_seed_stability))
    S, n_k = len(cells.strategies), len(cells.required_k)
    joint = joint_inputs(frame, n_k, S)
    projection = project_cells(cells)
    top_n = min(int(candidate_contribution_size), S)
    top_counts, maxima = run_root_bootstrap(engine, projection, weights, int(replicates), top_n, joint, range_size=range_size)
    enriched, summary = joint_tables(frame, maxima, cells.roots, int(replicates), float(joint_discrepancy_alpha))
    inclusion = top_n_inclusion_table(top_counts, cells.roots, cells.strategies, n_k, weights, int(replicates), top_n)
    return {"root_bootstrap_top_n_inclusion": inclusion, "root_discrepancies": enriched, "root_joint_discrepancy": summary}


# ---- the eight frames that are no bootstrap family, from one window call --------------------------------------------------------
BY_K_INT = ("raw_wins", "raw_exposures", "raw_attempted_exposures", "raw_completed_exposures", "raw_safety_limit_exposures", "raw_losses",
            "raw_declared_batches", "raw_batches", "excluded_zero_exposure_batch_cells")
ACROSS_COUNTS = ("raw_wins", "raw_attempted_exposures", "raw_completed_exposures", "raw_safety_limit_exposures", "raw_losses",
                 "raw_declared_batches", "raw_batches", "excluded_zero_exposure_batch_cells")
DIAGNOSTIC_FRAMES = ("performance_root_combination_across_k", "root_rank_stability", "root_top_n_stability", "root_control_movement",
                     "root_shortlist_changes", "root_matched_count_convergence", "root_half_drift")


def by_k_frame_name(k: int) -> str:
    return f"performance_root_combination_{int(k)}p"


def window_estimate(sums: Mapping, windows: Sequence[int], declared_batches: int, k: int, practical_delta: float) -> dict:
    """Every column of ``_estimate_matrix_cells`` (:437-498) that is computed, ``[S]`` each, for the scope made of ``windows`` (positions
    in ``sums``) with ``declared_batches`` rows in all: ``scope_from_windows`` plus the counts, the rates and the ``t.ppf`` interval."""
    from scipy.stats import t

    core = scope_from_windows(sums, windows, k, practical_delta)
    S = len(core["chance_delta"])
    total = {name: np.zeros(S, np.int64) for name in WINDOW_TOTALS}
    for i in windows:
        for name in WINDOW_TOTALS:
            total[name] += sums[name][i]
    wins, exposures, completed, safety, positive_batches = (total[name] for name in ("wins", "exposures", "completed", "safety", "positive_batches"))
    rates = wins / exposures
    mcse = core["batch_mcse"]
    interval_low, interval_high = np.full(S, np.nan, dtype=np.float64), np.full(S, np.nan, dtype=np.float64)
    eligible = positive_batches >= 2
    if np.any(eligible):
        critical = t.ppf(0.975, positive_batches[eligible] - 1)
        interval_low[eligible] = np.maximum(0.0, rates[eligible] - critical * mcse[eligible])
        interval_high[eligible] = np.minimum(1.0, rates[eligible] + critical * mcse[eligible])
    declared = np.full(S, int(declared_batches), np.int64)
    return {"raw_wins": wins, "raw_exposures": exposures, "raw_attempted_exposures": exposures, "raw_completed_exposures": completed,
            "raw_safety_limit_exposures": safety, "raw_losses": total["losses"], "raw_declared_batches": declared, "raw_batches": positive_batches,
            "excluded_zero_exposure_batch_cells": declared - positive_batches, "win_rate": rates, "win_rate_per_attempt": rates,
            "win_rate_given_completion": np.divide(wins, completed, out=np.full(S, np.nan, dtype=np.float64), where=completed > 0),
            "safety_limit_exposure_rate": safety / exposures, "chance_delta": core["chance_delta"], "batch_mcse": mcse,
            "batch_mc_precision_interval_low": interval_low, "batch_mc_precision_interval_high": interval_high,
            "practical_threshold_position": core["practical_threshold_position"]}


def by_k_schema():
    import pyarrow as pa

    floats = ("chance_baseline", "win_rate", "win_rate_per_attempt", "win_rate_given_completion", "safety_limit_exposure_rate", "chance_delta",
              "batch_mcse", "batch_mc_precision_interval_low", "batch_mc_precision_interval_high", "practical_delta")
    return pa.schema([("estimate_scope", pa.string()), ("root_seed", pa.int64()), ("k", pa.int64()), ("strategy", pa.int32()),
                      ("chance_baseline", pa.float64()), *[(name, pa.int64()) for name in BY_K_INT], ("batch_support_policy", pa.string()),
                      *[(name, pa.float64()) for name in floats[1:9]], ("practical_delta", pa.float64()),
                      ("practical_threshold_position", pa.string())])


def by_k_table(scoped: Sequence, strategies: np.ndarray, k: int, practical_delta: float):
    """The frame of one player count (:1036-1042): ``scoped`` = ``(scope, root or None, window_estimate(...))`` per scope in order."""
    import pyarrow as pa

    from .performance import RECTANGULAR_SUPPORT_POLICY

    schema = by_k_schema()
    S = len(strategies)
    columns = {name: [] for name in schema.names}
    for scope, root, est in scoped:
        fixed = {"estimate_scope": [scope] * S, "root_seed": [root] * S, "k": [int(k)] * S, "strategy": np.asarray(strategies).astype(np.int32).tolist(),
                 "chance_baseline": [1.0 / k] * S, "batch_support_policy": [RECTANGULAR_SUPPORT_POLICY] * S, "practical_delta": [float(practical_delta)] * S}
        for name in schema.names:
            columns[name] += fixed[name] if name in fixed else list(est[name]) if name == "practical_threshold_position" else est[name].tolist()
    arrays = [_nullable(columns[f.name]) if f.type == pa.float64() else pa.array(columns[f.name], type=f.type) for f in schema]
    return pa.Table.from_arrays(arrays, schema=schema)


def across_estimate(by_k: Mapping, required_k: Sequence[int], weights: Sequence[float], practical_delta: float, given=None) -> dict:
    """``_estimate_across_k`` (:516-593) for one scope: ``by_k[k]`` = ``window_estimate(...)``.  ``given``: ``(across_k_score,
    across_k_mcse)`` in place of the two ``np.dot`` columns (see the module docstring)."""
    from scipy.stats import norm

    ks = [int(k) for k in required_k]
    values = np.stack([by_k[k]["chance_delta"] for k in ks])
    if given is not None:
        score, error = (np.asarray(v, dtype=np.float64) for v in given)
    else:
        score, error = across_k_estimates(values, np.stack([by_k[k]["batch_mcse"] for k in ks]), weights)
    critical = float(norm.ppf(0.975))
    worst = np.argmin(values, axis=0)
    S = values.shape[1]
    out = {name: np.asarray([sum(int(by_k[k][name][s]) for k in ks) for s in range(S)], dtype=np.int64) for name in ACROSS_COUNTS}
    out.update({"across_k_score": score, "across_k_mcse": error, "across_k_mc_precision_interval_low": score - critical * error,
                "across_k_mc_precision_interval_high": score + critical * error, "minimum_chance_delta": values[worst, np.arange(S)],
                "worst_k": np.asarray(ks, dtype=np.int64)[worst],
                "practical_threshold_position": [threshold_position(float(v), float(practical_delta)) for v in score],
                "safety_limit_exposure_rate": np.asarray([int(f) / int(e) for f, e in zip(out["raw_safety_limit_exposures"].tolist(),
                                                                                          out["raw_attempted_exposures"].tolist())], dtype=np.float64)})
    return out


def across_schema():
    import pyarrow as pa

    return pa.schema([("estimate_scope", pa.string()), ("root_seed", pa.int64()), ("strategy", pa.int32()), ("required_k_count", pa.int64()),
                      ("support_k_count", pa.int64()), ("complete_support", pa.bool_()), *[(name, pa.int64()) for name in ACROSS_COUNTS],
                      ("k_aggregation_method", pa.string()), ("across_k_score", pa.float64()), ("across_k_mcse", pa.float64()),
                      ("across_k_mc_precision_interval_low", pa.float64()), ("across_k_mc_precision_interval_high", pa.float64()),
                      ("minimum_chance_delta", pa.float64()), ("worst_k", pa.int64()), ("practical_delta", pa.float64()),
                      ("practical_threshold_position", pa.string()), ("safety_limit_exposure_rate", pa.float64())])


def across_table(scoped: Sequence, strategies: np.ndarray, n_k: int, weights: Sequence[float], practical_delta: float):
    """The across-k frame (:1794-1798): ``scoped`` = ``(scope, root or None, across_estimate(...))`` per scope in order."""
    import pyarrow as pa

    schema = across_schema()
    S = len(strategies)
    columns = {name: [] for name in schema.names}
    for scope, root, est in scoped:
        fixed = {"estimate_scope": [scope] * S, "root_seed": [root] * S, "strategy": np.asarray(strategies).astype(np.int32).tolist(),
                 "required_k_count": [int(n_k)] * S, "support_k_count": [int(n_k)] * S, "complete_support": [True] * S,
                 "k_aggregation_method": [method_name(weights)] * S, "practical_delta": [float(practical_delta)] * S}
        for name in schema.names:
            columns[name] += fixed[name] if name in fixed else list(est[name]) if name == "practical_threshold_position" else est[name].tolist()
    arrays = [_nullable(columns[f.name]) if f.type == pa.float64() else pa.array(columns[f.name], type=f.type) for f in schema]
    return pa.Table.from_arrays(arrays, schema=schema)


def rank_vector(score: np.ndarray, strategies: np.ndarray) -> np.ndarray:
    """``_rank_map`` (:605-618) as int64 ``[S]`` aligned with ``strategies``: one-based ranks of a stable sort on (-score, strategy)."""
    order = np.lexsort((np.asarray(strategies, dtype=np.int64), -np.asarray(score, dtype=np.float64)))
    ranks = np.empty(len(order), dtype=np.int64)
    ranks[order] = np.arange(1, len(order) + 1, dtype=np.int64)
    return ranks


def rank_correlations(engine, rank_a: np.ndarray, rank_b: np.ndarray, want_kendall: bool = True) -> tuple:
    """``_correlations`` (:621-631): Spearman by ``structure_agreement.spearman``, Kendall's tau-b from the pair counts of
    ``engine.rank_concordance`` through ``kendall_from_counts``; ``(1.0, 1.0)`` below two strategies, NaN where scipy gives NaN."""
    from .structure_agreement import kendall_from_counts, spearman

    if len(rank_a) < 2:
        return 1.0, 1.0
    rho = spearman(rank_a, rank_b)
    tau = kendall_from_counts(engine.rank_concordance(rank_a, rank_b), len(rank_a)) if want_kendall else None
    return float("nan") if rho is None else rho, float("nan") if tau is None else tau


def shortlist_members(score: np.ndarray, delta: float) -> np.ndarray:
    score = np.asarray(score, dtype=np.float64)
    return score >= float(max(score.tolist())) - delta


def _table(columns: Mapping, kinds: Mapping):
    """An Arrow table of the named columns; float columns with NaN / None as nulls, as pandas hands them over."""
    import pyarrow as pa

    types = {"int64": pa.int64(), "int32": pa.int32(), "double": pa.float64(), "bool": pa.bool_(), "string": pa.string()}
    arrays = [_nullable(list(v)) if kinds[name] == "double" else pa.array(list(v), type=types[kinds[name]]) for name, v in columns.items()]
    return pa.Table.from_arrays(arrays, names=list(columns))


def rank_and_selection_tables(engine, roots: Sequence[int], strategies: np.ndarray, scores: Mapping, candidate_contribution_size: int,
                              controls: Sequence[int], delta_across_k: float | None) -> dict:
    """``_rank_and_selection_stability`` (:634-748): ``scores`` = the ``across_k_score`` of the three scopes in ``(root a, root b,
    combined)`` order, ``[S]`` each, aligned with ``strategies`` (ascending)."""
    import pyarrow as pa

    strategies = np.asarray(strategies, dtype=np.int64)
    S = len(strategies)
    score_a, score_b, score_c = (np.asarray(v, dtype=np.float64) for v in scores)
    rank_a, rank_b, rank_c = (rank_vector(v, strategies) for v in (score_a, score_b, score_c))
    rho, tau = rank_correlations(engine, rank_a, rank_b)
    movements = np.abs(rank_a - rank_b).astype(float)
    cutoff = min(int(candidate_contribution_size), S)
    top_movements = movements[rank_c <= cutoff]
    rank = _table({"root_a": [int(roots[0])], "root_b": [int(roots[1])], "strategy_count": [S], "spearman_rank_correlation": [rho],
                   "kendall_rank_correlation": [tau], "median_absolute_rank_movement": [float(np.median(movements))],
                   "p95_absolute_rank_movement": [float(np.quantile(movements, 0.95))],
                   "maximum_absolute_rank_movement": [float(movements.max(initial=0.0))], "combined_candidate_cutoff": [cutoff],
                   "combined_top_median_absolute_rank_movement": [float(np.median(top_movements))],
                   "combined_top_maximum_absolute_rank_movement": [float(top_movements.max(initial=0.0))]},
                  {"root_a": "int64", "root_b": "int64", "strategy_count": "int64", "combined_candidate_cutoff": "int64",
                   **{name: "double" for name in ("spearman_rank_correlation", "kendall_rank_correlation", "median_absolute_rank_movement",
                                                  "p95_absolute_rank_movement", "maximum_absolute_rank_movement",
                                                  "combined_top_median_absolute_rank_movement", "combined_top_maximum_absolute_rank_movement")}})
    top = {name: [] for name in ("requested_top_n", "effective_top_n", "root_overlap_count", "root_jaccard", "root_a_combined_overlap_count",
                                 "root_b_combined_overlap_count")}
    for top_n in sorted({10, 25, 50, int(candidate_contribution_size)}):
        effective = min(top_n, S)
        in_a, in_b, in_c = rank_a <= effective, rank_b <= effective, rank_c <= effective
        both, either = int(np.count_nonzero(in_a & in_b)), int(np.count_nonzero(in_a | in_b))
        for name, value in zip(top, (top_n, effective, both, both / either if either else 1.0, int(np.count_nonzero(in_a & in_c)),
                                     int(np.count_nonzero(in_b & in_c)))):
            top[name].append(value)
    top_n_table = _table(top, {name: "double" if name == "root_jaccard" else "int64" for name in top})
    position = {int(s): i for i, s in enumerate(strategies.tolist())}
    names = ("strategy", "root_a_rank", "root_b_rank", "combined_rank", "absolute_rank_movement", "root_a_score", "root_b_score", "combined_score",
             "raw_score_difference")
    control = {name: [] for name in names}
    for strategy in sorted({int(c) for c in controls}):
        if strategy not in position:
            raise ValueError(f"declared control {strategy} lacks complete two-root support")
        i = position[strategy]
        a, b = float(score_a[i]), float(score_b[i])
        for name, value in zip(names, (strategy, int(rank_a[i]), int(rank_b[i]), int(rank_c[i]), abs(int(rank_a[i]) - int(rank_b[i])), a, b,
                                       float(score_c[i]), a - b)):
            control[name].append(value)
    control_table = pa.table({}) if not control["strategy"] else _table(control, {
        "strategy": "int32", **{name: "int64" for name in names[1:5]}, **{name: "double" for name in names[5:]}})
    if delta_across_k is None:
        raise ValueError("screening.delta_across_k is required for shortlist stability")
    in_a, in_b, in_c = (shortlist_members(v, float(delta_across_k)) for v in (score_a, score_b, score_c))
    shortlist = _table({"strategy": strategies.astype(np.int32).tolist(), "root_a_shortlist": in_a.tolist(), "root_b_shortlist": in_b.tolist(),
                        "combined_shortlist": in_c.tolist(), "root_shortlist_changed": (in_a != in_b).tolist(),
                        "combined_changed_from_either_root": ((in_c != in_a) | (in_c != in_b)).tolist()},
                       {"strategy": "int32", **{name: "bool" for name in ("root_a_shortlist", "root_b_shortlist", "combined_shortlist",
                                                                          "root_shortlist_changed", "combined_changed_from_either_root")}})
    return {"root_rank_stability": rank, "root_top_n_stability": top_n_table, "root_control_movement": control_table,
            "root_shortlist_changes": shortlist}


CONVERGENCE_KINDS = {"cumulative_fraction": "double", "matched_batches_per_root_k": "int64", "root_spearman_rank_correlation": "double",
                     "root_kendall_rank_correlation": "double", "root_a_spearman_with_final_combined": "double",
                     "root_b_spearman_with_final_combined": "double", "partial_combined_spearman_with_final": "double",
                     "partial_combined_kendall_with_final": "double", "candidate_cutoff": "int64", "root_candidate_overlap_count": "int64",
                     "root_candidate_jaccard": "double", "shortlist_symmetric_difference_from_final": "int64",
                     "median_combined_interval_half_width": "double", "maximum_root_raw_discrepancy": "double", "interpretation": "string"}
DRIFT_KINDS = {"root_seed": "int64", "estimand_scope": "string", "k": "double", "strategy": "int32", "first_half_estimate": "double",
               "second_half_estimate": "double", "raw_difference": "double", "expected_mcse": "double", "standardized_drift": "double",
               "threshold_fraction": "double", "practical_threshold_position_changed": "bool", "interpretation": "string"}


def matched_count(minimum_batches: int, fraction: float) -> int:
    from math import ceil

    return min(int(minimum_batches), max(1, ceil(int(minimum_batches) * fraction)))


def diagnostic_tables(engine, cells: RootCells, candidate_contribution_size: int, practical_delta_by_k: Mapping | None,
                      delta_across_k: float | None, delta_seed_stability: float, k_aggregation_method: str = "equal-k",
                      declared_k_weights: Mapping | None = None, controls: Sequence[int] = (),
                      matched_count_fractions: Sequence[float] = (0.25, 0.5, 0.75, 1.0), stage_batch_bytes: int = DEFAULT_STAGE_BATCH_BYTES,
                      across_k: Mapping | None = None) -> tuple:
    """The eight frames of ``build_two_root_stability`` (:1761-1792) that are no bootstrap family, from ONE
    ``engine.root_window_estimates`` call over the stage's window list (``stage_windows``), and the ``ScopeEstimates`` the discrepancy
    chain continues from.  ``across_k``: ``{label: {scope: (across_k_score, across_k_mcse)}}`` in place of the ``np.dot`` columns, labels
    ``full``, ``matched_<count>`` and ``first_half_<root>`` / ``second_half_<root>`` (the tests feed a fixture's recorded columns)."""
    from scipy.stats import norm

    if practical_delta_by_k is None:
        raise ValueError("screening.practical_delta_by_k is required")
    if delta_across_k is None:
        raise ValueError("screening.delta_across_k is required")
    practical = {int(k): float(v) for k, v in practical_delta_by_k.items()}
    ks, (root_a, root_b) = list(cells.required_k), cells.roots
    missing = [k for k in ks if k not in practical]
    if missing:
        raise ValueError(f"screening.practical_delta_by_k is required for every player count; missing {missing}")
    weights = k_weights(k_aggregation_method, declared_k_weights, ks)
    ordered = cells.in_order()
    cell_of = {(root, k): i for i, (root, k) in enumerate((root, k) for root in cells.roots for k in ks)}
    counts = [len(m.wins) for m in ordered]
    for (root, k), i in cell_of.items():
        if counts[i] < 2:
            raise ValueError(f"root {root}, k={k} needs at least two batches for drift")
    strategies, S = cells.strategies, len(cells.strategies)
    windows, index = stage_windows(counts, S, int(stage_batch_bytes), matched_count_fractions)
    sums = engine.root_window_estimates([m.wins for m in ordered], [m.exposures for m in ordered], [m.completed for m in ordered],
                                        [m.safety for m in ordered], windows)
    scopes = (f"root_{root_a}", f"root_{root_b}", SCOPE_COMBINED)
    given = across_k or {}

    def scope_chain(label: str, rows) -> tuple:
        """The three scopes over rows ``[0, rows(cell))`` of every cell: ``(by_k {k: {scope: estimate}}, across {scope: estimate})``."""
        by_k = {}
        for k in ks:
            a, b = cell_of[(root_a, k)], cell_of[(root_b, k)]
            wa, wb = index[(a, 0, rows(a))], index[(b, 0, rows(b))]
            by_k[k] = {scopes[0]: window_estimate(sums, [wa], rows(a), k, practical[k]), scopes[1]: window_estimate(sums, [wb], rows(b), k, practical[k]),
                       scopes[2]: window_estimate(sums, [wa, wb], rows(a) + rows(b), k, practical[k])}
        across = {scope: across_estimate({k: by_k[k][scope] for k in ks}, ks, weights, delta_across_k, given.get(label, {}).get(scope)) for scope in scopes}
        return by_k, across

    by_k, across = scope_chain("full", lambda cell: counts[cell])
    seeds = (root_a, root_b, None)
    tables = {by_k_frame_name(k): by_k_table([(scope, seed, by_k[k][scope]) for scope, seed in zip(scopes, seeds)], strategies, k, practical[k]) for k in ks}
    tables["performance_root_combination_across_k"] = across_table([(scope, seed, across[scope]) for scope, seed in zip(scopes, seeds)], strategies,
                                                                   len(ks), weights, delta_across_k)
    final_scores = [across[scope]["across_k_score"] for scope in scopes]
    tables.update(rank_and_selection_tables(engine, cells.roots, strategies, final_scores, candidate_contribution_size, controls, delta_across_k))

    # _matched_count_convergence (:1429-1513)
    final_rank = rank_vector(final_scores[2], strategies)
    final_shortlist = shortlist_members(final_scores[2], float(delta_across_k))
    cutoff = min(int(candidate_contribution_size), S)
    minimum = min(counts)
    rows = {name: [] for name in CONVERGENCE_KINDS}
    for fraction in matched_count_fractions:
        matched = matched_count(minimum, fraction)
        _, partial = scope_chain(f"matched_{matched}", lambda cell: matched)
        score_a, score_b, score_c = (partial[scope]["across_k_score"] for scope in scopes)
        rank_a, rank_b, rank_c = (rank_vector(v, strategies) for v in (score_a, score_b, score_c))
        root_rho, root_tau = rank_correlations(engine, rank_a, rank_b)
        a_final, _ = rank_correlations(engine, rank_a, final_rank, want_kendall=False)
        b_final, _ = rank_correlations(engine, rank_b, final_rank, want_kendall=False)
        c_final_rho, c_final_tau = rank_correlations(engine, rank_c, final_rank)
        in_a, in_b = rank_a <= cutoff, rank_b <= cutoff
        both, either = int(np.count_nonzero(in_a & in_b)), int(np.count_nonzero(in_a | in_b))
        half_width = float(np.median(float(norm.ppf(0.975)) * partial[scopes[2]]["across_k_mcse"]))
        for name, value in zip(rows, (float(fraction), matched, root_rho, root_tau, a_final, b_final, c_final_rho, c_final_tau, cutoff, both,
                                      both / either, int(np.count_nonzero(shortlist_members(score_c, float(delta_across_k)) != final_shortlist)),
                                      half_width, float(np.abs(score_a - score_b).max()), "matched_count_convergence_not_additional_roots")):
            rows[name].append(value)
    tables["root_matched_count_convergence"] = _table(rows, CONVERGENCE_KINDS)

    # _half_drift (:1516-1628)
    drift = {name: [] for name in DRIFT_KINDS}
    ids = np.asarray(strategies).astype(np.int32).tolist()

    def drift_rows(root, scope_name, k, first, second, value, error):
        for s in range(S):
            one, two = float(first[value][s]), float(second[value][s])
            raw = one - two
            error_one, error_two = float(first[error][s]), float(second[error][s])
            expected = None if np.isnan(error_one) or np.isnan(error_two) else sqrt(error_one ** 2 + error_two ** 2)
            changed = first["practical_threshold_position"][s] != second["practical_threshold_position"][s]
            for name, item in zip(drift, (int(root), scope_name, k, ids[s], one, two, raw, expected, safe_standardized(raw, expected),
                                          abs(raw) / delta_seed_stability, changed, "within_root_drift_not_additional_root")):
                drift[name].append(item)

    for root in cells.roots:
        halves = {"first_half": {}, "second_half": {}}
        for k in ks:
            cell = cell_of[(root, k)]
            midpoint = counts[cell] // 2
            halves["first_half"][k] = window_estimate(sums, [index[(cell, 0, midpoint)]], midpoint, k, practical[k])
            halves["second_half"][k] = window_estimate(sums, [index[(cell, midpoint, counts[cell])]], counts[cell] - midpoint, k, practical[k])
            drift_rows(root, "by_k", k, halves["first_half"][k], halves["second_half"][k], "chance_delta", "batch_mcse")
        first, second = (across_estimate(halves[half], ks, weights, delta_across_k, given.get(f"{half}_{root}", {}).get(half))
                         for half in ("first_half", "second_half"))
        drift_rows(root, "across_k", None, first, second, "across_k_score", "across_k_mcse")
    tables["root_half_drift"] = _table(drift, DRIFT_KINDS)

    estimates = ScopeEstimates(scopes, {k: {scope: {name: by_k[k][scope][name] for name in ("chance_delta", "batch_mcse", "practical_threshold_position")}
                                            for scope in scopes} for k in ks},
                               {scope: {name: across[scope][name] for name in ("across_k_score", "across_k_mcse", "practical_threshold_position")}
                                for scope in scopes})
    return tables, estimates


def root_stability_diagnostic_tables(engine, cells: RootCells, replicates: int, candidate_contribution_size: int,
                                     practical_delta_by_k: Mapping | None, delta_across_k: float | None, delta_seed_stability: float,
                                     joint_discrepancy_alpha: float, k_aggregation_method: str = "equal-k",
                                     declared_k_weights: Mapping | None = None, controls: Sequence[int] = (),
                                     matched_count_fractions: Sequence[float] = (0.25, 0.5, 0.75, 1.0),
                                     stage_batch_bytes: int = DEFAULT_STAGE_BATCH_BYTES, range_size: int | None = None,
                                     across_k: Mapping | None = None) -> dict:
    """All eleven frames of the stage: the eight of ``diagnostic_tables`` and the three of ``root_stability_tables``, whose discrepancy
    chain takes its estimates from the same window call."""
    tables, estimates = diagnostic_tables(engine, cells, candidate_contribution_size, practical_delta_by_k, delta_across_k, delta_seed_stability,
                                          k_aggregation_method, declared_k_weights, controls, matched_count_fractions, stage_batch_bytes,
                                          across_k=across_k)
    tables.update(root_stability_tables(engine, cells, replicates, candidate_contribution_size, practical_delta_by_k, delta_across_k,
                                        delta_seed_stability, joint_discrepancy_alpha, k_aggregation_method, declared_k_weights,
                                        range_size=range_size, estimates=estimates))
    return tables
