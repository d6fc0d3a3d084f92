"""The performance stage's joint deterministic-batch bootstrap from the engine's per-batch seat statistics.

The reference (``src/farkle/analysis/performance.py``) materialises one ``performance_batch_matrix.npy`` per player count from the
all-player batch table (``_write_batch_matrix`` :163-227, dtype ``_BATCH_MATRIX_DTYPE`` :62-74, checks ``_validate_matrix_array``
:134-160), resamples the deterministic batches of every player count jointly (``_BootstrapRangeWriter.__call__`` :838-928: one
``.npy`` of replicate scores per range of 50 replicates) and reduces the ranges to ``performance_bootstrap.parquet`` and
``performance_control_contrasts.parquet`` (``_reduce_bootstrap_ranges`` :1013-1111; ``_joint_batch_resampling`` :715-833 states the
same in memory).  The inputs are two columns of the statistics the engine already holds per batch and strategy (``wins`` and
``exposures`` of ``backend.SEAT_STAT_NAMES``), the random numbers are coordinate streams the device already generates, and the
arithmetic is integer sums followed by a handful of float64 operations: ``Engine.performance_bootstrap``
(``fk_performance_bootstrap``, csrc/fk_bootstrap.h) reproduces it bit for bit.

This module holds what stays on the host: the matrix in the reference's layout (``BatchMatrix``), the projection the reference applies
before sampling (``project``: complete-support strategies, per player count the batches where every one of them has an exposure), the
frames (``bootstrap_tables``), the driver (``run_bootstrap``, ``write_bootstrap_range``) and a NumPy HOST STATEMENT of the device's
work (``host_bootstrap``: the real ``numpy.random.Generator(PCG64DXSM)`` behind ``random.coordinate_rng``), which is the oracle of the
tests and the engine behind their stub.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Mapping, Sequence

import numpy as np

from .backend import SEAT_STAT_NAMES
from .random import RandomPurpose, coordinate_rng

BATCH_MATRIX_DTYPE = np.dtype([("root_seed", "<i8"), ("deterministic_batch_id", "<i4"), ("strategy", "<i4"), ("raw_wins", "<i8"),
                               ("raw_player_game_exposures", "<i8"), ("raw_completed_player_game_exposures", "<i8"),
                               ("raw_safety_limit_player_game_exposures", "<i8"), ("raw_losses", "<i8")], align=False)  # :62-74
BOOTSTRAP_RANGE_SIZE = 50  # _BOOTSTRAP_RANGE_SIZE :75


def validate_matrix_array(matrix: np.ndarray, *, path, k: int) -> None:
    """``_validate_matrix_array`` (:134-160): the layout and the conservation laws of a canonical batch matrix."""
    if matrix.dtype != BATCH_MATRIX_DTYPE or matrix.ndim != 2 or not matrix.size:
        raise ValueError(f"{path} is not a canonical performance batch matrix")
    if np.unique(matrix["root_seed"]).size != 1:
        raise ValueError(f"{path} must contain exactly one root")
    strategies = matrix["strategy"][0]
    batches = matrix["deterministic_batch_id"][:, 0]
    if not np.all(matrix["strategy"] == strategies[np.newaxis, :]):
        raise ValueError(f"{path} has inconsistent strategy columns")
    if not np.all(matrix["deterministic_batch_id"] == batches[:, np.newaxis]):
        raise ValueError(f"{path} has inconsistent deterministic batch rows")
    if np.any(strategies < 0) or np.any(strategies[1:] <= strategies[:-1]):
        raise ValueError(f"{path} strategy IDs are not strictly increasing")
    if np.any(batches[1:] <= batches[:-1]):
        raise ValueError(f"{path} deterministic batch IDs are not strictly increasing")
    attempted, completed = matrix["raw_player_game_exposures"], matrix["raw_completed_player_game_exposures"]
    safety, wins, losses = matrix["raw_safety_limit_player_game_exposures"], matrix["raw_wins"], matrix["raw_losses"]
    if np.any(attempted < 0) or np.any(wins < 0) or np.any(wins > completed):
        raise ValueError(f"{path} contains impossible win/exposure counts for k={k}")
    if not np.array_equal(attempted, completed + safety):
        raise ValueError(f"{path} violates attempted exposure conservation")
    if not np.array_equal(losses, attempted - wins):
        raise ValueError(f"{path} violates all-participant loss conservation")


@dataclass
class BatchMatrix:
    """One player count's ``[batches][strategies]`` counts: rows in ascending deterministic batch id, columns in ascending strategy id."""

    root_seed: int
    k: int
    batch_ids: np.ndarray   # int32 [B]
    strategies: np.ndarray  # int32 [S]
    wins: np.ndarray        # int64 [B][S]
    exposures: np.ndarray
    completed: np.ndarray
    safety: np.ndarray

    @classmethod
    def from_seat_stats(cls, seat_stats, strategy_ids: Sequence[int], root_seed: int, k: int, batch_ids: Sequence[int],
                        columns: Sequence[str] = SEAT_STAT_NAMES) -> "BatchMatrix":
        """``seat_stats``: int64 ``[B][S][len(columns)]`` of the batches ``batch_ids``, table order; ``columns`` names its last axis
        (default: all of ``SEAT_STAT_NAMES``; the four counts used here are enough).  As the all-player batch
        table leaves out a strategy without an exposure in a batch (all_player.py) and the reference's matrix writer refuses a table
        that is not rectangular (:196-201), a strategy that sits in some batches and not in others is an error; one that never sits is
        not part of the matrix."""
        st = np.asarray(seat_stats, dtype=np.int64)
        col = {name: i for i, name in enumerate(columns)}
        ids = np.asarray(strategy_ids, dtype=np.int64)
        b_ids = np.asarray(batch_ids, dtype=np.int64)
        if st.ndim != 3 or st.shape[0] != len(b_ids) or st.shape[1] != len(ids) or st.shape[2] != len(col) or not len(b_ids):
            raise ValueError("seat_stats must be [batches][strategies][columns] with at least one batch")
        order_b, order_s = np.argsort(b_ids, kind="stable"), np.argsort(ids, kind="stable")
        st, ids, b_ids = st[order_b][:, order_s], ids[order_s], b_ids[order_b]
        present = st[:, :, col["exposures"]] > 0
        keep = present.any(axis=0)
        if not keep.any():
            raise ValueError("the batches hold no exposure")
        if not present[:, keep].all():
            raise ValueError(f"{k}p is missing declared rectangular strategy/batch cells: a strategy without an exposure in some "
                             "deterministic batch has no row in the all-player batch table")
        st, ids = st[:, keep], ids[keep]
        return cls(int(root_seed), int(k), b_ids.astype(np.int32), ids.astype(np.int32), st[:, :, col["wins"]].copy(),
                   st[:, :, col["exposures"]].copy(), st[:, :, col["completed_exposures"]].copy(),
                   st[:, :, col["safety_limit_exposures"]].copy())

    def to_reference_array(self) -> np.ndarray:
        m = np.zeros(self.wins.shape, dtype=BATCH_MATRIX_DTYPE)
        m["root_seed"] = self.root_seed
        m["deterministic_batch_id"] = self.batch_ids[:, np.newaxis]
        m["strategy"] = self.strategies[np.newaxis, :]
        m["raw_wins"], m["raw_player_game_exposures"] = self.wins, self.exposures
        m["raw_completed_player_game_exposures"], m["raw_safety_limit_player_game_exposures"] = self.completed, self.safety
        m["raw_losses"] = self.exposures - self.wins
        validate_matrix_array(m, path=f"{self.k}p batch matrix", k=self.k)
        return m

    @classmethod
    def from_reference_array(cls, matrix: np.ndarray, k: int, path="batch matrix") -> "BatchMatrix":
        validate_matrix_array(matrix, path=path, k=k)
        return cls(int(matrix["root_seed"][0, 0]), int(k), np.array(matrix["deterministic_batch_id"][:, 0], dtype=np.int32),
                   np.array(matrix["strategy"][0], dtype=np.int32), np.array(matrix["raw_wins"], dtype=np.int64),
                   np.array(matrix["raw_player_game_exposures"], dtype=np.int64),
                   np.array(matrix["raw_completed_player_game_exposures"], dtype=np.int64),
                   np.array(matrix["raw_safety_limit_player_game_exposures"], dtype=np.int64))

    def save(self, path) -> None:
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        tmp = path.with_name(path.name + ".tmp.npy")
        np.save(tmp, self.to_reference_array(), allow_pickle=False)
        tmp.replace(path)

    @classmethod
    def load(cls, path, k: int) -> "BatchMatrix":
        return cls.from_reference_array(np.load(path, mmap_mode="r", allow_pickle=False), k, path=path)


def complete_support_strategies(matrices: Mapping[int, BatchMatrix], required_k: Sequence[int]) -> np.ndarray:
    """Strategies with a column in the matrix of EVERY required player count, ascending (``_across_k_estimates`` :575-680: a
    strategy is complete when every per-k frame has it, and every matrix column has positive total exposure, :483-485)."""
    common = None
    for k in required_k:
        m = matrices[int(k)]
        if np.any(m.exposures.sum(axis=0, dtype=np.int64) <= 0):
            missing = m.strategies[m.exposures.sum(axis=0, dtype=np.int64) <= 0].tolist()
            raise ValueError(f"strategies have no positive exposure support: {missing[:10]}")
        ids = set(int(v) for v in m.strategies)
        common = ids if common is None else common & ids
    out = np.asarray(sorted(common or ()), dtype=np.int64)
    if not len(out):
        raise ValueError("no strategies have complete configured k support")
    return out


@dataclass
class Projection:
    """What the sampler sees (:849-871): per required player count the eligible batches' wins / exposures over the strategy columns."""

    root_seed: int
    required_k: tuple
    strategies: np.ndarray  # int64 [S] ascending
    wins: list              # per k: int64 [B_k][S]
    exposures: list
    eligible: list          # per k: positions of the eligible batches in the matrix


def project(matrices: Mapping[int, BatchMatrix], required_k: Sequence[int], strategies: Sequence[int] | None = None) -> Projection:
    required = tuple(int(k) for k in required_k)
    ids = complete_support_strategies(matrices, required) if strategies is None else np.asarray(strategies, dtype=np.int64)
    roots = {int(matrices[k].root_seed) for k in required}
    if len(roots) != 1:
        raise ValueError(f"single-root performance inputs disagree on root: {sorted(roots)}")
    wins, exposures, eligible = [], [], []
    for k in required:
        m = matrices[k]
        available = m.strategies.astype(np.int64)
        positions = np.searchsorted(available, ids)
        if np.any(positions >= len(available)) or not np.array_equal(available[np.minimum(positions, len(available) - 1)], ids):
            raise ValueError(f"{k}p batch matrix lacks complete configured strategy support")
        e = m.exposures[:, positions]
        rows = np.flatnonzero(np.all(e > 0, axis=1))
        if not rows.size:
            raise ValueError("joint resampling has no positive-exposure batch vectors")
        wins.append(np.ascontiguousarray(m.wins[:, positions][rows]))
        exposures.append(np.ascontiguousarray(e[rows]))
        eligible.append(rows)
    return Projection(roots.pop(), required, ids, wins, exposures, eligible)


# ---- the host statement -------------------------------------------------------------------------------------------------------
def bounded_draws(bit_generator, bound: int, n: int) -> np.ndarray:
    """``Generator(bit_generator).integers(0, bound, size=n)`` restated on the raw 64-bit outputs, as the device draws (numpy's
    ``buffered_bounded_lemire_uint32``): 32-bit words, the low half of an output first; ``m = word * bound``; only when
    ``low32(m) < bound`` the threshold ``(2**32 - bound) % bound`` is computed and words are redrawn while ``low32(m)`` is below it;
    result ``m >> 32``.  ``bound == 1`` draws nothing.  1 <= bound <= 2**32 - 1."""
    bound = int(bound)
    if not 1 <= bound <= 2 ** 32 - 1:
        raise ValueError("bound must be in [1, 2**32 - 1]")
    out = np.zeros(int(n), dtype=np.int64)
    if bound == 1:
        return out
    buffered: list[int] = []

    def word() -> int:
        if buffered:
            return buffered.pop()
        raw = int(bit_generator.random_raw())
        buffered.append(raw >> 32)
        return raw & 0xFFFFFFFF

    for i in range(int(n)):
        m = word() * bound
        if (m & 0xFFFFFFFF) < bound:
            threshold = (2 ** 32 - bound) % bound
            while (m & 0xFFFFFFFF) < threshold:
                m = word() * bound
        out[i] = m >> 32
    return out


def resample_counts(root_seed: int, k: int, replicate: int, n_batches: int) -> np.ndarray:
    """The multiplicities of one (replicate, player count) stream (:893-903), by numpy's own generator."""
    rng = coordinate_rng(RandomPurpose.BOOTSTRAP, root_seed=int(root_seed), k=int(k), replicate_index=int(replicate))
    selected = rng.integers(0, n_batches, size=n_batches)
    return np.bincount(selected, minlength=n_batches).astype(np.int64, copy=False)


def host_scores(root_seed: int, ks: Sequence[int], wins: Sequence[np.ndarray], exposures: Sequence[np.ndarray], start: int,
                stop: int) -> np.ndarray:
    """Replicate score rows ``[stop - start][S]`` (:886-927)."""
    S = wins[0].shape[1]
    scores = np.zeros((max(stop - start, 0), S), dtype=np.float64)
    for row, replicate in enumerate(range(start, stop)):
        out = scores[row]
        for k, w, e in zip(ks, wins, exposures):
            counts = resample_counts(root_seed, k, replicate, len(w))
            total_wins = counts @ np.asarray(w, dtype=np.int64)  # exact int64
            total_exposures = counts @ np.asarray(e, dtype=np.int64)
            if np.any(total_exposures <= 0):
                raise ValueError("joint batch resampling produced zero complete-support exposure")
            out += total_wins / total_exposures - 1.0 / int(k)
        out /= len(ks)
    return scores


def host_bootstrap(root_seed: int, ks, wins, exposures, replicate_begin: int, replicate_end: int, top_n: int, delta: float,
                   controls=(), want_scores: bool = True, contrast_sum=None, contrast_square_sum=None) -> dict:
    """``Engine.performance_bootstrap`` in NumPy: the same arguments, the same result (:1038-1057 per replicate)."""
    W = [np.asarray(m, dtype=np.int64) for m in wins]
    E = [np.asarray(m, dtype=np.int64) for m in exposures]
    S = W[0].shape[1]
    if not 0 <= int(top_n) <= S:
        raise ValueError("top_n must be in [0, S]")
    ctrl = [int(c) for c in controls]
    if any(not 0 <= c < S for c in ctrl):
        raise ValueError("control column outside [0, S)")
    for w, e in zip(W, E):
        if np.any(w < 0) or np.any(e < 0):
            raise ValueError("negative count")
    scores = host_scores(root_seed, ks, W, E, int(replicate_begin), int(replicate_end))
    columns = np.arange(S, dtype=np.int64)
    rank_sum, rank_sq = np.zeros(S, np.int64), np.zeros(S, np.int64)
    top, shortlist = np.zeros(S, np.int64), np.zeros(S, np.int64)
    csum = np.zeros((len(ctrl), S)) if contrast_sum is None else np.array(contrast_sum, dtype=np.float64).reshape(len(ctrl), S)
    csq = np.zeros((len(ctrl), S)) if contrast_square_sum is None else np.array(contrast_square_sum, dtype=np.float64).reshape(len(ctrl), S)
    for row in scores:
        order = np.lexsort((columns, -row))
        ranks = np.empty(S, dtype=np.int64)
        ranks[order] = np.arange(1, S + 1)
        rank_sum += ranks
        rank_sq += ranks * ranks
        top[order[:int(top_n)]] += 1
        shortlist += row >= row.max() - float(delta)
        for position, index in enumerate(ctrl):
            contrasts = row - row[index]
            csum[position] += contrasts
            csq[position] += contrasts * contrasts
    return {"scores": scores if want_scores else None, "rank_sum": rank_sum, "rank_square_sum": rank_sq, "top_counts": top,
            "shortlist_counts": shortlist, "contrast_sum": csum, "contrast_square_sum": csq}


# ---- driver and frames ----------------------------------------------------------------------------------------------------------
@dataclass
class BootstrapSums:
    replicates: int
    rank_sum: np.ndarray
    rank_square_sum: np.ndarray
    top_counts: np.ndarray
    shortlist_counts: np.ndarray
    contrast_sum: np.ndarray
    contrast_square_sum: np.ndarray


def run_bootstrap(engine, projection: Projection, replicates: int, top_n: int, delta: float, control_indices: Sequence[int],
                  range_size: int | None = None) -> BootstrapSums:
    """All replicates through ``engine.performance_bootstrap`` (``range_size``: replicates per call, default all in one — the device
    blocks the range itself; the contrast sums are carried from call to call, so any split gives the same bits)."""
    S = len(projection.strategies)
    step = int(range_size) if range_size else max(int(replicates), 1)
    counters = [np.zeros(S, np.int64) for _ in range(4)]
    csum = csq = None
    for start in range(0, int(replicates), step):
        res = engine.performance_bootstrap(projection.root_seed, projection.required_k, projection.wins, projection.exposures, start,
                                           min(start + step, int(replicates)), top_n, delta, controls=control_indices, want_scores=False,
                                           contrast_sum=csum, contrast_square_sum=csq)
        for total, name in zip(counters, ("rank_sum", "rank_square_sum", "top_counts", "shortlist_counts")):
            total += res[name]
        csum, csq = res["contrast_sum"], res["contrast_square_sum"]
    if csum is None:
        csum = csq = np.zeros((len(control_indices), S))
    return BootstrapSums(int(replicates), *counters, np.asarray(csum), np.asarray(csq))


def equal_k_scores(matrices: Mapping[int, BatchMatrix], required_k: Sequence[int], strategies: np.ndarray) -> np.ndarray:
    """``equal_k_score`` of the complete-support strategies (:489-490 ``rates - chance`` over ALL batches of a player count, :645-649
    ``float(deltas.mean())`` over the required player counts)."""
    deltas = np.zeros((len(strategies), len(required_k)), dtype=np.float64)
    for j, k in enumerate(required_k):
        m = matrices[int(k)]
        positions = np.searchsorted(m.strategies.astype(np.int64), strategies)
        wins = m.wins[:, positions].sum(axis=0, dtype=np.int64)
        exposures = m.exposures[:, positions].sum(axis=0, dtype=np.int64)
        deltas[:, j] = wins / exposures - 1.0 / int(k)
    return np.asarray([float(np.array(row, dtype=np.float64).mean()) for row in deltas], dtype=np.float64)


def bootstrap_schema():
    import pyarrow as pa

    return pa.schema([("root_seed", pa.int64()), ("strategy", pa.int32()), ("bootstrap_replicates", pa.int64()),
                      ("bootstrap_rank_mean", pa.float64()), ("bootstrap_rank_sd", pa.float64()), ("top_n_size", pa.int64()),
                      ("top_n_inclusion_probability", pa.float64()), ("shortlist_delta", pa.float64()),
                      ("shortlist_inclusion_probability", pa.float64())])


def contrast_schema():
    import pyarrow as pa

    return pa.schema([("root_seed", pa.int64()), ("strategy", pa.int32()), ("control_strategy", pa.int32()),
                      ("observed_equal_k_contrast", pa.float64()), ("bootstrap_contrast_mean", pa.float64()),
                      ("bootstrap_contrast_sd", pa.float64()), ("bootstrap_replicates", pa.int64())])


def bootstrap_tables(sums: BootstrapSums, strategies: np.ndarray, root_seed: int, top_n: int, delta: float, controls: Sequence[int],
                     observed: np.ndarray):
    """The two frames of ``_reduce_bootstrap_ranges`` (:1058-1110) as Arrow tables: column names, order, types (strategy columns in
    the reference's canonical strategy id type, int32, ``_write_frame`` :1307-1314) and float expressions as there.  ``controls``:
    sorted control strategy ids; ``observed``: ``equal_k_scores`` of ``strategies``."""
    import pyarrow as pa

    S = len(strategies)
    if max(int(sums.rank_square_sum.max(initial=0)), int(sums.rank_sum.max(initial=0))) >= 2 ** 53:
        raise ValueError("rank sums beyond 2**53 are not exact in the reference's float64 accumulators")
    divisor = float(sums.replicates)
    with np.errstate(divide="ignore", invalid="ignore"):
        rank_mean = sums.rank_sum.astype(np.float64) / divisor
        rank_variance = np.maximum(sums.rank_square_sum.astype(np.float64) / divisor - rank_mean * rank_mean, 0.0)
        boot = pa.Table.from_pydict({
            "root_seed": np.full(S, int(root_seed), np.int64), "strategy": np.asarray(strategies).astype(np.int32),
            "bootstrap_replicates": np.full(S, sums.replicates, np.int64), "bootstrap_rank_mean": rank_mean,
            "bootstrap_rank_sd": np.sqrt(rank_variance), "top_n_size": np.full(S, int(top_n), np.int64),
            "top_n_inclusion_probability": sums.top_counts / divisor, "shortlist_delta": np.full(S, float(delta), np.float64),
            "shortlist_inclusion_probability": sums.shortlist_counts / divisor}, schema=bootstrap_schema())
        ctrl = np.asarray(list(controls), dtype=np.int64)
        if len(ctrl):
            index = np.searchsorted(strategies, ctrl)
            means = (sums.contrast_sum / divisor).reshape(-1)
            variances = np.maximum(sums.contrast_square_sum / divisor - (sums.contrast_sum / divisor) ** 2, 0.0).reshape(-1)
            observed_contrasts = np.concatenate([observed - observed[i] for i in index])
            strategy_column, control_column = np.tile(strategies, len(ctrl)), np.repeat(ctrl, S)
        else:
            means = variances = observed_contrasts = np.zeros(0, np.float64)
            strategy_column = control_column = np.zeros(0, np.int64)
        contrasts = pa.Table.from_pydict({
            "root_seed": np.full(len(strategy_column), int(root_seed), np.int64), "strategy": strategy_column.astype(np.int32),
            "control_strategy": control_column.astype(np.int32), "observed_equal_k_contrast": observed_contrasts,
            "bootstrap_contrast_mean": means, "bootstrap_contrast_sd": np.sqrt(variances),
            "bootstrap_replicates": np.full(len(strategy_column), sums.replicates, np.int64)}, schema=contrast_schema())
    return boot, contrasts


def resolve_controls(controls: Sequence[int], strategies: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Sorted unique control ids and their columns (:1031-1035); a control without complete support is an error."""
    ctrl = np.asarray(sorted(set(int(c) for c in controls)), dtype=np.int64)
    missing = sorted(set(ctrl.tolist()).difference(np.asarray(strategies).tolist()))
    if missing:
        raise ValueError(f"declared controls lack complete k support: {missing}")
    return ctrl, np.searchsorted(strategies, ctrl).astype(np.int32)


def performance_bootstrap_tables(engine, matrices: Mapping[int, BatchMatrix], required_k: Sequence[int], replicates: int,
                                 candidate_contribution_size: int, delta: float | None, controls: Sequence[int],
                                 range_size: int | None = None):
    """From the batch matrices of a root to the two frames: projection, ``engine.performance_bootstrap``, reduction."""
    if delta is None:
        raise ValueError("screening.delta_across_k is required for shortlist resampling")
    if int(replicates) < 1:
        raise ValueError("screening.bootstrap_replicates must be positive")
    required = sorted(int(k) for k in required_k)
    projection = project(matrices, required)
    ctrl, index = resolve_controls(controls, projection.strategies)
    top_n = min(int(candidate_contribution_size), len(projection.strategies))
    sums = run_bootstrap(engine, projection, replicates, top_n, float(delta), index, range_size=range_size)
    observed = equal_k_scores(matrices, required, projection.strategies)
    return bootstrap_tables(sums, projection.strategies, projection.root_seed, top_n, float(delta), ctrl, observed)


def write_bootstrap_range(engine, matrix_paths: Sequence, required_k: Sequence[int], strategies: Sequence[int], root_seed: int,
                          start: int, stop: int, path) -> None:
    """What the reference's ``_BootstrapRangeWriter(matrix_paths, required_k, strategies, root_seed, ...)`` writes for the unit
    ``(start, stop)``: a ``.npy`` of float64 ``[stop - start][len(strategies)]`` replicate scores (:838-928), computed by
    ``engine.performance_bootstrap``.  The seam a reference maintainer binds."""
    matrices = {int(k): BatchMatrix.load(p, int(k)) for k, p in zip(required_k, matrix_paths)}
    projection = project(matrices, [int(k) for k in required_k], strategies=np.asarray(strategies, dtype=np.int64))
    res = engine.performance_bootstrap(int(root_seed), projection.required_k, projection.wins, projection.exposures, int(start), int(stop),
                                       0, 0.0, controls=(), want_scores=True)
    out = np.lib.format.open_memmap(path, mode="w+", dtype=np.dtype("<f8"), shape=(int(stop) - int(start), len(projection.strategies)))
    out[:] = res["scores"]
    out.flush()
    del out

