"""Designed inputs of the performance stage's point estimates (fk_performance_by_k, fk_performance_across_k), built vectorised and
shared by tests/test_performance_host.py, tests/test_performance_gpu.py and tools/gen_performance_golden.py.

By k.  Column lengths ``B_SIZES`` sit on every seam of NumPy's pairwise order (below 8: sequential; 8: the eight accumulators start; 9
and 130: a tail; 128 / 129: one block or the first split; 257, 1 100: two and more levels), column counts ``S_SIZES`` around the
wavefront and the workgroup.  A batch row's rate is of order 0.1 or of order 1e-12, alternating down a column, so an addition in
another order rounds differently (``naive_sum_differs`` holds the cases to that).  Zero-exposure cells: none; one per column; all but
one (count 1, no mcse); all but two.

Across k.  Pareto sets over an integer grid, scaled per coordinate by alternating powers of ten (a monotone map keeps the order and
makes the row sums order-dependent), at ``N_SIZES`` = around the device's tile of 128 rows.
"""
from __future__ import annotations

import numpy as np

B_SIZES = (1, 2, 7, 8, 9, 16, 127, 128, 129, 130, 257, 1100)
S_SIZES = (1, 63, 64, 65, 257)
ZERO_PATTERNS = ("none", "one", "all_but_one", "all_but_two")
TILE = 128  # fkp::PT
N_SIZES = (1, TILE - 1, TILE, TILE + 1)
D_SIZES = (1, 2, 3, 8, 16)
PARETO_KINDS = ("chain", "antichain", "duplicates", "late_dominator", "last_tile_dominator", "equal_but_one")
MAXIMIN_KINDS = ("equal", "inside", "outside")


def by_k_case(B: int, S: int, zero: str = "none", seed: int = 0) -> dict:
    """Four int64 ``[B][S]`` matrices that satisfy the reference's conservation laws."""
    rng = np.random.default_rng([B, S, ZERO_PATTERNS.index(zero), seed])
    exposures = rng.integers(10 ** 12, 2 * 10 ** 12, size=(B, S), dtype=np.int64)
    safety = rng.integers(0, 4, size=(B, S), dtype=np.int64)
    large = (np.arange(B)[:, None] + np.arange(S)[None, :]) % 2 == 0
    wins = np.where(large, rng.integers(10 ** 11, 5 * 10 ** 11, size=(B, S), dtype=np.int64), rng.integers(1, 10, size=(B, S), dtype=np.int64))
    rows, cols = np.arange(B)[:, None], np.arange(S)[None, :]
    first, second = cols % B, (cols + B // 2 + 1) % B  # the rows that stay positive (distinct when B >= 2)
    if zero == "none" or B == 1:
        empty = np.zeros((B, S), dtype=bool)
    elif zero == "one":
        empty = rows == (7 * cols + 3) % B
    elif zero == "all_but_one":
        empty = rows != first
    elif zero == "all_but_two":
        empty = (rows != first) & (rows != second)
    else:
        raise ValueError(zero)
    exposures[empty] = safety[empty] = wins[empty] = 0
    return {"wins": wins, "exposures": exposures, "completed": exposures - safety, "safety": safety}


def zero_column_case(B: int = 9, S: int = 65, column: int = 64) -> dict:
    """A whole column without exposure: the refusal."""
    case = by_k_case(B, S)
    for name in case:
        case[name][:, column] = 0
    return case


def naive_sum(values: np.ndarray) -> float:
    total = 0.0
    for v in values.tolist():
        total += v
    return total


def naive_sum_differs(case: dict) -> bool:
    """Whether a left-to-right sum of some column's rates differs from NumPy's: the case can tell two summation orders apart."""
    w, e = case["wins"], case["exposures"]
    for s in range(w.shape[1]):
        positive = e[:, s] > 0
        rates = w[positive, s].astype(np.float64) / e[positive, s]
        if naive_sum(rates) != float(np.add.reduce(rates)):
            return True
    return False


def _scale(grid: np.ndarray) -> np.ndarray:
    d = grid.shape[1]
    factors = np.where(np.arange(d) % 2 == 0, 1e-3, 1e-15) * (1.0 + np.arange(d) / 7.0)
    return grid.astype(np.float64) * factors[None, :]


def pareto_case(kind: str, n: int, d: int, seed: int = 0) -> np.ndarray:
    """float64 ``[n][d]`` chance deltas, rows in ascending strategy id."""
    rng = np.random.default_rng([PARETO_KINDS.index(kind), n, d, seed])
    i = np.arange(n)
    if kind == "chain":  # every row is dominated by the next
        grid = np.repeat(i[:, None], d, axis=1) - n // 2
    elif kind == "antichain":  # nobody is dominated (d = 1: all equal)
        grid = np.zeros((n, d), dtype=np.int64)
        if d >= 2:
            grid[:, 0], grid[:, 1] = i, -i
    elif kind == "duplicates":  # rows 2j and 2j + 1 are the same point; points on a coarse grid dominate each other often
        grid = rng.integers(-3, 4, size=(n, d))
        grid[1::2] = grid[0:(n // 2) * 2:2]
    elif kind == "late_dominator":  # row b > a equals row a but for a larger last coordinate: equal first coordinate, larger id
        grid = rng.integers(-50, 50, size=(n, d))
        if n >= 2 and d >= 2:
            a, b = n // 3, n - 1 - n // 5
            grid[b] = grid[a]
            grid[b, d - 1] += 1
    elif kind == "last_tile_dominator":  # an antichain whose first row is dominated by the last row alone
        grid = np.zeros((n, d), dtype=np.int64)
        if d >= 2:
            grid[:, 0], grid[:, 1] = 2 * i, -2 * i
        if n >= 2:
            grid[n - 1] = grid[0] + 1
            if d >= 2:
                grid[n - 1, 1] = grid[0, 1]  # (equal there, larger elsewhere; beside every other row of the antichain)
    elif kind == "equal_but_one":  # all coordinates 0 but one: rows that share it form a chain, the others are incomparable
        grid = np.zeros((n, d), dtype=np.int64)
        grid[i, i % d] = i // d + 1
    else:
        raise ValueError(kind)
    return _scale(np.asarray(grid, dtype=np.int64))


def variances_case(n: int, d: int, seed: int = 0) -> np.ndarray:
    """Squared mcse values of alternating size; a NaN here and there (a column with fewer than two positive batches)."""
    rng = np.random.default_rng([77, n, d, seed])
    v = rng.random((n, d)) * np.where((np.arange(n)[:, None] + np.arange(d)[None, :]) % 2 == 0, 1e-6, 1e-18)
    if n >= 3:
        v[n // 2, d - 1] = np.nan
    return v


def maximin_case(kind: str, n: int = 130, d: int = 3) -> tuple[np.ndarray, int]:
    """Deltas whose largest minimum is shared or nearly shared by rows 37 and 129, and the leader the reference names."""
    deltas = pareto_case("antichain", n, d) - 1.0  # every minimum far below
    best = 0.015625
    low, high = 37, 129
    deltas[low], deltas[high] = best + 0.25, best + 0.25
    deltas[high, d - 1] = best
    if kind == "equal":
        deltas[low, 0], leader = best, low
    elif kind == "inside":  # 5e-16 below the best: within the tolerance, the smaller id leads
        deltas[low, 0], leader = best - 5e-16, low
    elif kind == "outside":  # 2e-15 below: the best alone
        deltas[low, 0], leader = best - 2e-15, high
    else:
        raise ValueError(kind)
    assert deltas[low, 0] != best or kind == "equal"
    return deltas, leader


def across_cases():
    """(name, deltas, variances) of every Pareto and maximin case."""
    for kind in PARETO_KINDS:
        for d in D_SIZES:
            for n in N_SIZES:
                yield f"{kind}-n{n}-d{d}", pareto_case(kind, n, d), variances_case(n, d)
    for kind in MAXIMIN_KINDS:
        deltas, _ = maximin_case(kind)
        yield f"maximin-{kind}", deltas, variances_case(*deltas.shape)


# ---- the golden subset (tools/gen_performance_golden.py records the reference's results on these) ----
GOLDEN_ROOT = 11
GOLDEN_EXTRA = 500  # a strategy that sits at two players only: incomplete support
GOLDEN_STRATEGIES = (1, 4, 7, 10, 13, 16)
GOLDEN_K = {2: (130, "one"), 3: (9, "all_but_two"), 5: (8, "none")}  # k -> (batches, zero pattern)
GOLDEN_PARETO = tuple((kind, n, d) for kind in PARETO_KINDS for n, d in ((TILE + 1, 3), (TILE - 1, 8), (TILE, 1)))
GOLDEN_SCREENING = {"resolution_delta": 0.03, "practical_delta_by_k": {2: 0.02, 3: 0.2, 5: 0.01}, "delta_across_k": 0.05,
                    "candidate_contribution_size": 4, "controls": [4, 13], "mandatory_diagnostics": [16]}


def golden_matrices(complete_only: bool) -> dict:
    """k -> (batch ids, strategy ids, the four matrices); ``complete_only`` drops the strategy that sits at two players only."""
    out = {}
    for k, (B, zero) in GOLDEN_K.items():
        ids = list(GOLDEN_STRATEGIES) + ([GOLDEN_EXTRA] if k == 2 and not complete_only else [])
        case = by_k_case(B, len(GOLDEN_STRATEGIES) + 1, zero, seed=k)
        if k == 5:  # one column with a single positive batch: no mcse at five players, hence none across k
            for name in case:
                case[name][1:, 2] = 0
        out[k] = (list(range(0, 2 * B, 2)), ids, {name: m[:, :len(ids)].copy() for name, m in case.items()})
    return out


def golden_bootstrap_columns(strategies) -> dict:
    """A bootstrap table to merge with (the reference's columns, performance_bootstrap.bootstrap_schema), values from the ids."""
    ids = np.asarray(strategies, dtype=np.int64)
    n = len(ids)
    return {"root_seed": np.full(n, GOLDEN_ROOT, np.int64), "strategy": ids.astype(np.int32), "bootstrap_replicates": np.full(n, 64, np.int64),
            "bootstrap_rank_mean": 1.0 + (ids % 5) / 4.0, "bootstrap_rank_sd": (ids % 3) / 8.0, "top_n_size": np.full(n, 4, np.int64),
            "top_n_inclusion_probability": (ids % 4) / 4.0, "shortlist_delta": np.full(n, 0.05), "shortlist_inclusion_probability": (ids % 7) / 8.0}
