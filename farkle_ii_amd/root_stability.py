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
                          range_size: int | None = None, across_k: Mapping | None = None) -> dict:
    """From the checked cells to the three frames ``root_bootstrap_top_n_inclusion``, ``root_discrepancies`` (enriched) and
    ``root_joint_discrepancy``: estimate chain, one ``engine.root_stability_bootstrap`` pass for both families, reductions."""
    if int(replicates) < 1:
        raise ValueError("screening.bootstrap_replicates must be positive")
    weights = k_weights(k_aggregation_method, declared_k_weights, cells.required_k)
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
