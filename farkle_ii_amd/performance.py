"""The performance stage's point estimates from the batch matrices of a root: the tables the joint batch bootstrap
(performance_bootstrap.py) is the uncertainty for.

The reference (``src/farkle/analysis/performance.py``) estimates every player count from its ``performance_batch_matrix.npy``
(``_estimate_one_k_matrix`` :425-542: column totals, the batch-to-batch standard error of the win rate over the batches with an
exposure, Wilson and t intervals), combines the player counts with equal weight over the strategies every one of them has
(``_across_k_estimates`` :575-687: ``equal_k_score``, ``equal_k_mcse``, the worst player count, Pareto membership by an incrementally
maintained frontier ``_pareto_membership`` :547-572, the maximin leader) and ``analysis/screening.py`` merges both with the bootstrap
table into the descriptive screening frame (``_build_screening_frame`` :32-90).  The sums over batches, the sums over player counts and
the all-pairs dominance test run on the device: ``Engine.performance_by_k`` (``fk_performance_by_k``) and
``Engine.performance_across_k`` (``fk_performance_across_k``, csrc/fk_performance.h), in NumPy's own summation order, so every float
below is the reference's bit for bit.

This module holds what stays on the host: the square roots, the division by ``n - 1``, scipy's quantiles and the Wilson interval (S
values per player count); the frames, column for column and type for type as the reference writes them (``by_k_frame``,
``across_k_frame``, ``screening_frame``, ``screening_payload``); and a NumPy HOST STATEMENT of both device passes (``host_by_k``,
``host_across_k``), which is the oracle of the tests and the engine behind their stub.

Left out: the player-count effect diagnostics (``_player_count_effect_diagnostics``, ``player_count_effects.parquet``), the
reference's artifact sidecars and stage stamps beyond what ``farkle run --sidecars`` writes for the neighbouring files, and TrueSkill
(the ``trueskill_rank`` of ``--agreement --candidate-membership`` stays the caller's; ``win_rate_rank`` is ``score_order_position``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Mapping, Sequence

import numpy as np

from .performance_bootstrap import BatchMatrix

RECTANGULAR_SUPPORT_POLICY = ("require_declared_strategy_by_batch_cartesian_support; exclude_zero-exposure cells from univariate estimates and "
                              "zero-containing vectors from joint resampling")  # analysis/batch_support.py:12-16
MAXIMIN_ATOL = 1e-15
MAX_PLAYER_COUNTS = 16  # fkp::MAX_D
COUNT_COLUMNS = ("raw_wins", "raw_attempted_exposures", "raw_completed_exposures", "raw_safety_limit_exposures", "raw_losses",
                 "raw_declared_batches", "raw_batches", "excluded_zero_exposure_batch_cells")  # :605-614
SCREENING_INTERPRETATION = ("Descriptive finite-grid screening evidence only; practical bands are not tests of equality, final tiers, or "
                            "unique-best decisions.")  # analysis/screening.py:146-149


# ---- the host statement -------------------------------------------------------------------------------------------------------
def host_by_k(k: int, wins, exposures, completed, safety) -> dict:
    """``Engine.performance_by_k`` in NumPy: the same arguments, the same result, the same refusals (as ValueError).  The float sums
    are NumPy's own reductions over the compacted rate vector, the statements ``np.std(rates, ddof=1)`` is made of (:474-479)."""
    W, E, C, F = (np.asarray(m, dtype=np.int64) for m in (wins, exposures, completed, safety))
    if int(k) < 1:
        raise ValueError(f"player count k = {int(k)}")
    if W.ndim != 2 or not W.size or any(m.shape != W.shape for m in (E, C, F)):
        raise ValueError(f"{k}p: the four count matrices are [batches][S] of one shape, one batch and one strategy at least")
    if np.any(W < 0) or np.any(E < 0) or np.any(C < 0) or np.any(F < 0):
        raise ValueError(f"{k}p: a negative count")
    if np.any(W > C):
        raise ValueError(f"{k}p: wins > completed: impossible win/exposure counts")
    if not np.array_equal(E, C + F):
        raise ValueError(f"{k}p: exposures != completed + safety: attempted exposure conservation")
    totals = {name: m.sum(axis=0, dtype=np.int64) for name, m in (("wins", W), ("exposures", E), ("completed", C), ("safety", F))}
    if np.any(totals["exposures"] <= 0):
        raise ValueError(f"{k}p: strategies have no positive exposure support: column {int(np.flatnonzero(totals['exposures'] <= 0)[0])}")
    S = W.shape[1]
    positive_batches, rate_sum, ssd = np.zeros(S, np.int64), np.zeros(S, np.float64), np.zeros(S, np.float64)
    for s in range(S):
        positive = E[:, s] > 0
        count = int(np.count_nonzero(positive))
        rates = W[positive, s].astype(np.float64) / E[positive, s]
        positive_batches[s] = count
        rate_sum[s] = np.add.reduce(rates)
        x = rates - rate_sum[s] / count
        ssd[s] = np.add.reduce(x * x)
    return {**totals, "losses": totals["exposures"] - totals["wins"], "positive_batches": positive_batches, "rate_sum": rate_sum, "ssd": ssd}


def squared_mcse(mcse) -> np.ndarray:
    """``mcse ** 2`` as the reference squares it (:646-648): Python's float power, element by element.  That is libm's ``pow``, which
    is not the IEEE product for about one value in 1 200 — so the squares are taken here, on the host, and the device sums them."""
    values = np.asarray(mcse, dtype=np.float64)
    return np.asarray([v ** 2 for v in values.reshape(-1).tolist()], dtype=np.float64).reshape(values.shape)


def pareto_members(deltas: np.ndarray) -> np.ndarray:
    """Row i is a member unless some row is >= in every coordinate and > in at least one (all pairs; equal rows dominate nothing)."""
    values = np.asarray(deltas, dtype=np.float64)
    member = np.ones(len(values), dtype=bool)
    for i, point in enumerate(values):
        member[i] = not np.any(np.all(values >= point, axis=1) & np.any(values > point, axis=1))
    return member


def host_across_k(deltas, variances) -> dict:
    """``Engine.performance_across_k`` in NumPy: the same arguments, the same result, the same refusals (as ValueError)."""
    D, V = np.asarray(deltas, dtype=np.float64), np.asarray(variances, dtype=np.float64)
    if D.ndim != 2 or D.shape != V.shape or not D.shape[0]:
        raise ValueError("deltas and variances are [n][d] arrays of one shape, one row at least")
    if not 1 <= D.shape[1] <= MAX_PLAYER_COUNTS:
        raise ValueError(f"d = {D.shape[1]}: 1 to {MAX_PLAYER_COUNTS} required player counts")
    if not np.all(np.isfinite(D)):
        raise ValueError("a chance delta is not finite")
    if np.any(V < 0.0) or np.any(np.isinf(V)):
        raise ValueError("a variance is negative or infinite")
    delta_sum = np.asarray([np.add.reduce(np.array(row, dtype=np.float64)) for row in D], dtype=np.float64)
    variance_sum = np.asarray([np.add.reduce(np.array(row, dtype=np.float64)) for row in V], dtype=np.float64)
    worst = np.argmin(D, axis=1).astype(np.int32)
    minimum = D[np.arange(len(D)), worst]
    best = float(minimum.max())
    leader = int(np.flatnonzero(np.isclose(minimum, best, rtol=0.0, atol=MAXIMIN_ATOL))[0])
    return {"delta_sum": delta_sum, "variance_sum": variance_sum, "minimum": minimum, "worst_index": worst,
            "pareto_member": pareto_members(D), "leader_row": leader}


class HostEngine:
    """The host statement behind the engine seam (the two calls the frames make)."""

    def performance_by_k(self, k, wins, exposures, completed, safety):
        return host_by_k(k, wins, exposures, completed, safety)

    def performance_across_k(self, deltas, variances):
        return host_across_k(deltas, variances)


# ---- per player count ---------------------------------------------------------------------------------------------------------------
def wilson_ci(k: int, n: int, z: float) -> tuple[float, float]:
    """``utils/stats.py: wilson_ci`` :93-138 with ``z = norm.ppf(1 - alpha / 2)`` taken once by the caller."""
    if n <= 0:
        raise ValueError("n must be positive")
    if not 0 <= k <= n:
        raise ValueError("k must be between 0 and n (inclusive)")
    proportion = k / n
    z2 = z * z
    denom = 1.0 + z2 / n
    center = proportion + z2 / (2.0 * n)
    margin = z * math.sqrt((proportion * (1.0 - proportion) + z2 / (4.0 * n)) / n)
    lower = float(max(0.0, min(1.0, (center - margin) / denom)))
    upper = float(max(0.0, min(1.0, (center + margin) / denom)))
    return (upper if lower > upper else lower), upper


@dataclass
class ByK:
    """One player count's estimates, one entry per strategy column (ascending strategy id): the columns of ``by_k_frame``."""

    root_seed: int
    k: int
    strategies: np.ndarray
    columns: dict


def estimate_by_k(engine, matrix: BatchMatrix, resolution_delta: float, practical_delta: float) -> ByK:
    """``_estimate_one_k_matrix`` (:425-542) with its sums over batches from ``engine.performance_by_k``."""
    from scipy.stats import norm, t

    k = int(matrix.k)
    sums = engine.performance_by_k(k, matrix.wins, matrix.exposures, matrix.completed, matrix.safety)
    wins, exposures, completed, safety = (np.asarray(sums[name], dtype=np.int64) for name in ("wins", "exposures", "completed", "safety"))
    count = np.asarray(sums["positive_batches"], dtype=np.int64)
    S, batch_count = len(wins), int(matrix.wins.shape[0])
    mcse = np.full(S, np.nan, dtype=np.float64)
    enough = count >= 2
    with np.errstate(divide="ignore", invalid="ignore"):
        # np.std(rates, ddof=1) / sqrt(count): sqrt(ssd / (count - 1)), then the division (:479)
        mcse[enough] = np.sqrt(np.asarray(sums["ssd"], dtype=np.float64)[enough] / (count[enough] - 1)) / np.sqrt(count[enough].astype(np.float64))
    rates = wins / exposures
    chance = 1.0 / k
    z = norm.ppf(1.0 - 0.05 / 2.0)
    wilson = [wilson_ci(int(w), int(e), z) for w, e in zip(wins, exposures)]
    wilson_low = np.asarray([v[0] for v in wilson], dtype=np.float64)
    wilson_high = np.asarray([v[1] for v in wilson], dtype=np.float64)
    widths = wilson_high - wilson_low
    interval_low, interval_high = np.full(S, np.nan), np.full(S, np.nan)
    finite = np.isfinite(mcse)
    if np.any(finite):
        critical = t.ppf(0.975, count[finite] - 1)
        interval_low[finite] = np.maximum(0.0, rates[finite] - critical * mcse[finite])
        interval_high[finite] = np.minimum(1.0, rates[finite] + critical * mcse[finite])
    columns = {
        "root_seed": np.full(S, int(matrix.root_seed), np.int64), "k": np.full(S, k, np.int64),
        "strategy": np.asarray(matrix.strategies).astype(np.int32), "chance_baseline": np.full(S, chance), "raw_wins": wins,
        "raw_exposures": exposures, "raw_attempted_exposures": exposures, "raw_completed_exposures": completed,
        "raw_safety_limit_exposures": safety, "raw_losses": np.asarray(sums["losses"], dtype=np.int64),
        "raw_declared_batches": np.full(S, batch_count, np.int64), "raw_batches": count,
        "excluded_zero_exposure_batch_cells": batch_count - count, "batch_support_policy": [RECTANGULAR_SUPPORT_POLICY] * S,
        "win_rate_per_attempt": rates, "win_rate": rates,
        "win_rate_given_completion": np.divide(wins, completed, out=np.full(S, np.nan, dtype=np.float64), where=completed > 0),
        "safety_limit_exposure_rate": safety / exposures, "chance_delta": rates - chance, "wilson_interval_low": wilson_low,
        "wilson_interval_high": wilson_high, "wilson_interval_width": widths,
        "screening_resolution_delta": np.full(S, float(resolution_delta)), "practical_delta_by_k": np.full(S, float(practical_delta)),
        "wilson_resolution_met": widths <= float(resolution_delta), "batch_mcse": mcse, "batch_interval_low": interval_low,
        "batch_interval_high": interval_high}
    return ByK(int(matrix.root_seed), k, np.asarray(matrix.strategies, dtype=np.int64), columns)


def by_k_schema():
    import pyarrow as pa

    i8, f8 = pa.int64(), pa.float64()
    return pa.schema([("root_seed", i8), ("k", i8), ("strategy", pa.int32()), ("chance_baseline", f8), ("raw_wins", i8), ("raw_exposures", i8),
                      ("raw_attempted_exposures", i8), ("raw_completed_exposures", i8), ("raw_safety_limit_exposures", i8), ("raw_losses", i8),
                      ("raw_declared_batches", i8), ("raw_batches", i8), ("excluded_zero_exposure_batch_cells", i8),
                      ("batch_support_policy", pa.string()), ("win_rate_per_attempt", f8), ("win_rate", f8), ("win_rate_given_completion", f8),
                      ("safety_limit_exposure_rate", f8), ("chance_delta", f8), ("wilson_interval_low", f8), ("wilson_interval_high", f8),
                      ("wilson_interval_width", f8), ("screening_resolution_delta", f8), ("practical_delta_by_k", f8),
                      ("wilson_resolution_met", pa.bool_()), ("batch_mcse", f8), ("batch_interval_low", f8), ("batch_interval_high", f8)])


def _table(columns: Mapping, schema):
    """Arrow table of NumPy columns; a NaN is a null, as in the reference's frames once pandas has handed them to Arrow."""
    import pyarrow as pa

    return pa.Table.from_arrays([pa.array(columns[f.name], type=f.type, from_pandas=True) for f in schema], schema=schema)


def by_k_frame(engine, matrix: BatchMatrix, resolution_delta: float, practical_delta: float):
    """``performance_by_k`` of one player count as the reference writes it; returns ``(table, ByK)``."""
    estimates = estimate_by_k(engine, matrix, resolution_delta, practical_delta)
    return _table(estimates.columns, by_k_schema()), estimates


# ---- across player counts -----------------------------------------------------------------------------------------------------------
def across_k_schema(any_incomplete: bool):
    """With a strategy of incomplete support the count columns and ``worst_k`` hold nulls, and pandas has made them float64."""
    import pyarrow as pa

    i8, f8, b = pa.int64(), pa.float64(), pa.bool_()
    counts = f8 if any_incomplete else i8
    return pa.schema([("root_seed", i8), ("strategy", pa.int32()), ("required_k_count", i8), ("support_k_count", i8), ("complete_support", b),
                      *[(name, counts) for name in COUNT_COLUMNS], ("safety_limit_exposure_rate", f8), ("practical_delta_across_k", f8),
                      ("equal_k_score", f8), ("equal_k_mcse", f8), ("equal_k_interval_low", f8), ("equal_k_interval_high", f8),
                      ("minimum_chance_delta", f8), ("worst_k", counts), ("pareto_member", b), ("maximin_value", f8), ("maximin_leader", b)])


def across_k_frame(engine, by_k: Mapping[int, ByK], required_k: Sequence[int], practical_delta: float):
    """``performance_across_k`` (``_across_k_estimates`` :575-687) with its sums, minima, Pareto front and maximin leader from
    ``engine.performance_across_k``.  Returns ``(table, complete strategies, their [n][d] chance deltas)``."""
    from scipy.stats import norm

    required = [int(k) for k in required_k]
    if not required or len(required) > MAX_PLAYER_COUNTS:
        raise ValueError(f"1 to {MAX_PLAYER_COUNTS} required player counts")
    roots = {int(by_k[k].root_seed) for k in required}
    if len(roots) != 1:
        raise ValueError(f"single-root performance inputs disagree on root: {sorted(roots)}")
    all_strategies = np.asarray(sorted(set().union(*(set(by_k[k].strategies.tolist()) for k in required))), dtype=np.int64)
    n_all, d = len(all_strategies), len(required)
    present = np.zeros((n_all, d), dtype=bool)
    position = np.zeros((n_all, d), dtype=np.int64)
    for j, k in enumerate(required):
        ids = by_k[k].strategies
        at = np.minimum(np.searchsorted(ids, all_strategies), len(ids) - 1)
        present[:, j] = ids[at] == all_strategies
        position[:, j] = at
    complete = present.all(axis=1)
    rows = np.flatnonzero(complete)
    if not len(rows):
        raise ValueError("no strategies have complete configured k support")
    n = len(rows)
    deltas, mcse = np.zeros((n, d)), np.zeros((n, d))
    counts = {name: np.zeros(n, dtype=np.int64) for name in COUNT_COLUMNS}
    for j, k in enumerate(required):
        at = position[rows, j]
        deltas[:, j] = by_k[k].columns["chance_delta"][at]
        mcse[:, j] = by_k[k].columns["batch_mcse"][at]
        for name in COUNT_COLUMNS:
            counts[name] += np.asarray(by_k[k].columns[name], dtype=np.int64)[at]
    res = engine.performance_across_k(deltas, squared_mcse(mcse))
    score = np.asarray(res["delta_sum"], dtype=np.float64) / d                 # float(deltas.mean())
    equal_mcse = np.sqrt(np.asarray(res["variance_sum"], dtype=np.float64) / (d ** 2))  # sqrt(np.sum(variances) / len(required_k) ** 2)
    critical = float(norm.ppf(0.975))
    member = np.asarray(res["pareto_member"], dtype=bool)
    leader = np.zeros(n, dtype=bool)
    leader[int(res["leader_row"])] = True
    any_incomplete = n < n_all

    def spread(values, fill, dtype):
        out = np.full(n_all, fill, dtype=dtype)
        out[rows] = values
        return out

    count_type = np.float64 if any_incomplete else np.int64
    safety_rate = np.asarray([int(s) / int(a) for s, a in zip(counts["raw_safety_limit_exposures"], counts["raw_attempted_exposures"])])
    columns = {
        "root_seed": np.full(n_all, roots.pop(), np.int64), "strategy": all_strategies.astype(np.int32),
        "required_k_count": np.full(n_all, d, np.int64), "support_k_count": present.sum(axis=1).astype(np.int64), "complete_support": complete,
        **{name: spread(counts[name], np.nan if any_incomplete else 0, count_type) for name in COUNT_COLUMNS},
        "safety_limit_exposure_rate": spread(safety_rate, np.nan, np.float64),
        "practical_delta_across_k": np.full(n_all, float(practical_delta)), "equal_k_score": spread(score, np.nan, np.float64),
        "equal_k_mcse": spread(equal_mcse, np.nan, np.float64), "equal_k_interval_low": spread(score - critical * equal_mcse, np.nan, np.float64),
        "equal_k_interval_high": spread(score + critical * equal_mcse, np.nan, np.float64),
        "minimum_chance_delta": spread(res["minimum"], np.nan, np.float64),
        "worst_k": spread(np.asarray(required, dtype=np.int64)[np.asarray(res["worst_index"], dtype=np.int64)], np.nan if any_incomplete else 0,
                          count_type),
        "pareto_member": spread(member, False, bool), "maximin_value": spread(res["minimum"], np.nan, np.float64),
        "maximin_leader": spread(leader, False, bool)}
    return _table(columns, across_k_schema(any_incomplete)), all_strategies[rows], deltas


# ---- descriptive screening ----------------------------------------------------------------------------------------------------------
def screening_frame(across, bootstrap, by_k: Mapping[int, object], player_counts: Sequence[int], candidate_contribution_size: int,
                    delta_across_k: float | None, practical_delta_by_k: Mapping[int, float], controls: Sequence[int],
                    mandatory_diagnostics: Sequence[int]):
    """``_build_screening_frame`` (analysis/screening.py:32-90) over the three Arrow tables (``by_k``: player count -> the by-k
    table): the across-k rows merged with the bootstrap table, ordered by (``equal_k_score`` descending, ``strategy``), with the
    practical bands across and per player count."""
    import pyarrow as pa

    a = {name: across.column(name).to_numpy(zero_copy_only=False) for name in across.schema.names}
    if not np.all(a["complete_support"]):
        incomplete = a["strategy"][~a["complete_support"].astype(bool)].astype(int).tolist()
        raise ValueError(f"descriptive screening requires complete configured k support; incomplete strategies: {incomplete[:20]}")
    boot = {name: bootstrap.column(name).to_numpy(zero_copy_only=False) for name in bootstrap.schema.names}
    keys = lambda cols: list(zip(np.asarray(cols["root_seed"]).tolist(), np.asarray(cols["strategy"]).tolist()))  # noqa: E731
    if len(set(keys(boot))) != len(boot["strategy"]) or len(set(keys(a))) != len(a["strategy"]):
        raise ValueError("Merge keys are not unique: not a one-to-one merge")
    boot_at = {key: i for i, key in enumerate(keys(boot))}
    kept = np.asarray([i for i, key in enumerate(keys(a)) if key in boot_at], dtype=np.int64)  # (an inner merge in the left frame's order)
    take_boot = np.asarray([boot_at[key] for key in keys(a) if key in boot_at], dtype=np.int64)
    order = np.lexsort((a["strategy"][kept], -a["equal_k_score"][kept]))
    left, right = kept[order], take_boot[order]
    n = len(left)
    fields = [(f.name, f.type, a[f.name][left]) for f in across.schema]
    fields += [(f.name, f.type, boot[f.name][right]) for f in bootstrap.schema if f.name not in ("root_seed", "strategy")]
    score, strategy = a["equal_k_score"][left], a["strategy"][left]
    position = np.arange(1, n + 1, dtype=np.int64)
    leader_score = float(score.max())
    fields += [("score_order_position", pa.int64(), position),
               ("observed_top_n", pa.bool_(), position <= min(int(candidate_contribution_size), n)),
               ("within_across_k_practical_band", pa.bool_(), score >= (leader_score - float(delta_across_k or 0.0))),
               ("declared_control", pa.bool_(), np.isin(strategy, np.asarray(list(controls), dtype=np.int64))),
               ("mandatory_diagnostic", pa.bool_(), np.isin(strategy, np.asarray(list(mandatory_diagnostics), dtype=np.int64)))]
    every = np.ones(n, dtype=bool)
    for k in player_counts:
        table = by_k[int(k)]
        ids = table.column("strategy").to_numpy(zero_copy_only=False)
        at = {(int(r), int(s)): i for i, (r, s) in enumerate(zip(table.column("root_seed").to_pylist(), ids.tolist()))}
        missing = [int(s) for r, s in zip(a["root_seed"][left].tolist(), strategy.tolist()) if (int(r), int(s)) not in at]
        if missing:
            raise ValueError(f"{k}p performance estimates lack screened strategies: {missing[:20]}")
        take = np.asarray([at[(int(r), int(s))] for r, s in zip(a["root_seed"][left].tolist(), strategy.tolist())], dtype=np.int64)
        delta = table.column("chance_delta").to_numpy(zero_copy_only=False)[take]
        band = delta >= (float(delta.max()) - float(practical_delta_by_k[int(k)]))
        every &= band
        fields += [(f"chance_delta_k{k}", pa.float64(), delta),
                   (f"win_rate_k{k}", pa.float64(), table.column("win_rate").to_numpy(zero_copy_only=False)[take]),
                   (f"raw_exposures_k{k}", pa.int64(), table.column("raw_exposures").to_numpy(zero_copy_only=False)[take]),
                   (f"within_k{k}_practical_band", pa.bool_(), band)]
    fields.append(("within_every_k_practical_band", pa.bool_(), every))
    schema = pa.schema([(name, kind) for name, kind, _ in fields])
    return _table({name: values for name, _, values in fields}, schema)


def screening_payload(screening, player_counts: Sequence[int], artifact: str = "descriptive_screening.parquet") -> dict:
    """The ``descriptive_screening.json`` payload (analysis/screening.py:144-156)."""
    member = np.asarray(screening.column("pareto_member").to_pylist(), dtype=bool)
    leader = np.asarray(screening.column("maximin_leader").to_pylist(), dtype=bool)
    strategy = screening.column("strategy").to_pylist()
    return {"artifact": artifact, "interpretation": SCREENING_INTERPRETATION, "player_counts": [int(k) for k in player_counts],
            "strategy_count": screening.num_rows, "pareto_count": int(member.sum()), "maximin_leader": int(strategy[int(np.flatnonzero(leader)[0])]),
            "control_count": int(np.count_nonzero(screening.column("declared_control").to_pylist())),
            "mandatory_diagnostic_count": int(np.count_nonzero(screening.column("mandatory_diagnostic").to_pylist()))}


def win_rate_ranks(screening) -> dict:
    """``{strategy: win_rate_rank}``: ``score_order_position``, the rank ``--agreement --candidate-membership`` asks the caller for."""
    return {int(s): int(p) for s, p in zip(screening.column("strategy").to_pylist(), screening.column("score_order_position").to_pylist())}
