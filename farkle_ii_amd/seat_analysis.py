"""The reference's seat-analysis stage (analysis/seat_analysis.py) from the device's counts, without rows.

``fk_tournament_run_seat_counts`` delivers, per deterministic batch, strategy and seat, the wins / completed exposures / safety-limit
exposures (``SeatCounts``) and, at k = 2, per unordered strategy pair the six additive sums of the mirrored-game pairing
(``MirroredPairs``).  This module holds the host statement of both over rows (``from_rows``: the literal two-queue loop of
``_MirroredPartitionWriter.__call__`` :618-714 is the statement the device's closed form is tested against), their merge over
shuffle ranges, and the frames the stage publishes, with the reference's columns, order, dtypes and float operation order:

    batch_counts_table   _COUNT_SCHEMA :42-54, rows of _iter_seat_count_tables :170-235 (only cells with an exposure)
    within_k_frames      _within_k_frames :326-376 (strategy x seat, and the population per seat)
    standardized_frames  _standardized_frames :393-499 (declared-weight effects and the exposure mixture over common support)
    selfplay_frame       _game_diagnostics :502-540 (all seats one strategy: with unique IDs only k = 1)
    mirrored_frame       the output schema of _write_mirrored_diagnostic :765-779
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

WINS, COMPLETED, SAFETY = 0, 1, 2  # columns of the device's counts
PAIR_COLUMNS = ("paired_mirrored_games", "p1_win_difference_sum", "games_completed", "games_safety_limit", "unpaired_forward_games",
                "unpaired_reverse_games")
FORWARD, REVERSE, SAFETY_GAME = 0, 1, 2  # orientation codes of a mirrored-game record


def id_ranks(strategy_ids, S: int | None = None) -> np.ndarray:
    """uint16 ``[S]``: the rank of every table index by strategy ID.  Duplicate IDs are refused: the pairing is by ID."""
    ids = np.asarray(strategy_ids, dtype=np.int64).reshape(-1)
    if S is not None and len(ids) != S:
        raise ValueError(f"strategy_ids has {len(ids)} entries for a table of {S}")
    if len(np.unique(ids)) != len(ids):
        raise ValueError("seat analysis needs unique strategy IDs: two table rows share one")
    rank = np.empty(len(ids), dtype=np.uint16)
    rank[np.argsort(ids, kind="stable")] = np.arange(len(ids), dtype=np.uint16)
    return rank


def pair_two_queue(orientation, p1_win) -> tuple[int, int, int, int, int, int]:
    """One (batch, pair) segment in row order -> ``PAIR_COLUMNS``, by the reference's two FIFO queues: a completed game is paired
    with the oldest waiting game of the opposite orientation, or waits."""
    forward: list[int] = []
    reverse: list[int] = []
    f_head = r_head = matched = difference = completed = safety = 0
    for o, p1 in zip(orientation, p1_win):
        o, p1 = int(o), int(p1)
        if o == SAFETY_GAME:
            safety += 1
            continue
        completed += 1
        if o == FORWARD:
            if r_head < len(reverse):
                difference += p1 - reverse[r_head]
                r_head += 1
                matched += 1
            else:
                forward.append(p1)
        elif f_head < len(forward):
            difference += forward[f_head] - p1
            f_head += 1
            matched += 1
        else:
            reverse.append(p1)
    return matched, difference, completed, safety, len(forward) - f_head, len(reverse) - r_head


def pair_closed_form(orientation, p1_win) -> tuple[int, int, int, int, int, int]:
    """The same six values without queues (what the device computes): the queues are never both non-empty, so the i-th completed
    forward game meets the i-th completed reverse game and m = min(nF, nR) pairs form."""
    o, p1 = np.asarray(orientation, dtype=np.int64), np.asarray(p1_win, dtype=np.int64)
    f, r = p1[o == FORWARD], p1[o == REVERSE]
    m = min(len(f), len(r))
    return m, int(f[:m].sum() - r[:m].sum()), len(f) + len(r), int((o == SAFETY_GAME).sum()), len(f) - m, len(r) - m


@dataclass
class SeatCounts:
    """int64 ``counts [n_batches][S][k][3]`` (wins, completed, safety-limit exposures) of batches ``first_batch ...``."""

    k: int
    first_batch: int
    counts: np.ndarray

    @classmethod
    def from_engine(cls, res: dict, k: int, first_batch: int = 0) -> "SeatCounts":
        return cls(int(k), int(first_batch), np.asarray(res["seat_counts"], dtype=np.int64))

    @classmethod
    def from_rows(cls, rows: np.ndarray, k: int, S: int, shuffles_per_batch: int, first_batch: int = 0) -> "SeatCounts":
        """Host statement over ``backend.row_dtype(k)`` rows in (shuffle, game) order of a range that starts on a batch boundary."""
        gps = S // k
        n = len(rows)
        batch = (np.arange(n) // gps) // max(int(shuffles_per_batch), 1)
        out = np.zeros((int(batch.max()) + 1 if n else 0, S, k, 3), dtype=np.int64)
        completed = rows["status"] == 0
        for seat in range(k):
            strat = rows["seats"][:, seat]["strategy"].astype(np.int64)
            np.add.at(out[:, :, seat, WINS], (batch, strat), (completed & (rows["winner_seat"] == seat)).astype(np.int64))
            np.add.at(out[:, :, seat, COMPLETED], (batch, strat), completed.astype(np.int64))
            np.add.at(out[:, :, seat, SAFETY], (batch, strat), (~completed).astype(np.int64))
        return cls(int(k), int(first_batch), out)

    def merge(self, other: "SeatCounts") -> "SeatCounts":
        """Counts of two ranges that each start on a batch boundary: batches both hold add."""
        if self.k != other.k or self.counts.shape[1:] != other.counts.shape[1:]:
            raise ValueError("seat counts of different tables or player counts do not merge")
        lo = min(self.first_batch, other.first_batch)
        hi = max(self.first_batch + len(self.counts), other.first_batch + len(other.counts))
        out = np.zeros((hi - lo,) + self.counts.shape[1:], dtype=np.int64)
        for part in (self, other):
            out[part.first_batch - lo:part.first_batch - lo + len(part.counts)] += part.counts
        return SeatCounts(self.k, lo, out)


@dataclass
class MirroredPairs:
    """``ids`` int64 ``[n][2]`` (strategy IDs, a < b, rows ascending) and ``sums`` int64 ``[n][6]`` (``PAIR_COLUMNS``)."""

    ids: np.ndarray
    sums: np.ndarray

    @classmethod
    def empty(cls) -> "MirroredPairs":
        return cls(np.zeros((0, 2), np.int64), np.zeros((0, 6), np.int64))

    @classmethod
    def from_engine(cls, res: dict, strategy_ids) -> "MirroredPairs":
        ids = np.asarray(strategy_ids, dtype=np.int64)
        return cls(ids[np.asarray(res["pair_index"], dtype=np.int64).reshape(-1, 2)], np.asarray(res["pair_sums"], dtype=np.int64).reshape(-1, 6))

    @classmethod
    def from_rows(cls, rows: np.ndarray, S: int, shuffles_per_batch: int, strategy_ids) -> "MirroredPairs":
        """Host statement over k = 2 rows in (shuffle, game) order of a range that starts on a batch boundary: per (batch, pair)
        the two-queue loop in row order, summed over the batches."""
        ids = np.asarray(strategy_ids, dtype=np.int64)
        id_ranks(ids, S)
        gps = S // 2
        segments: dict = {}
        for i, row in enumerate(rows):
            first, second = int(ids[row["seats"][0]["strategy"]]), int(ids[row["seats"][1]["strategy"]])
            if first == second:
                continue
            a, b = min(first, second), max(first, second)
            key = (a, b, (i // gps) // max(int(shuffles_per_batch), 1))
            if int(row["status"]) != 0:
                segments.setdefault(key, []).append((SAFETY_GAME, 0))
            else:
                segments.setdefault(key, []).append((REVERSE if first == b else FORWARD, int(row["winner_seat"] == 0)))
        totals: dict = {}
        for (a, b, _batch), games in segments.items():
            v = pair_two_queue([g[0] for g in games], [g[1] for g in games])
            t = totals.setdefault((a, b), [0] * 6)
            for j in range(6):
                t[j] += v[j]
        keys = sorted(totals)
        return cls(np.asarray(keys, dtype=np.int64).reshape(-1, 2), np.asarray([totals[key] for key in keys], dtype=np.int64).reshape(-1, 6))

    def merge(self, other: "MirroredPairs") -> "MirroredPairs":
        """Pairs of two ranges of whole batches (every sum is additive over batches)."""
        ids = np.concatenate([self.ids, other.ids])
        sums = np.concatenate([self.sums, other.sums])
        if not len(ids):
            return MirroredPairs.empty()
        uniq, inverse = np.unique(ids, axis=0, return_inverse=True)
        out = np.zeros((len(uniq), 6), dtype=np.int64)
        np.add.at(out, np.asarray(inverse).reshape(-1), sums)
        return MirroredPairs(uniq.astype(np.int64), out)


# ------------------------------------------------------------------------------------------------ frames
def _rate(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """One float64 division per row (int64 / int64 as pandas divides them); 0 / 0 is NaN as there."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return num.astype(np.float64) / den.astype(np.float64)


def batch_counts_table(counts: SeatCounts, strategy_ids, root_seed: int):
    """``seat_batch_counts.parquet``: one row per (batch, strategy ID, seat) with an exposure, in that order."""
    import pyarrow as pa

    ids = np.asarray(strategy_ids, dtype=np.int64)
    id_ranks(ids, counts.counts.shape[1])
    c = counts.counts[:, np.argsort(ids, kind="stable")]  # strategies in ascending ID
    sorted_ids = np.sort(ids)
    exposures = c[..., COMPLETED] + c[..., SAFETY]
    b, s, q = np.nonzero(exposures)
    n = len(b)
    return pa.table({
        "root_seed": pa.array(np.full(n, int(root_seed), np.int64)), "k": pa.array(np.full(n, counts.k, np.int16)),
        "deterministic_batch_id": pa.array((b + counts.first_batch).astype(np.int32)), "strategy": pa.array(sorted_ids[s].astype(np.int32)),
        "seat": pa.array((q + 1).astype(np.int16)), "raw_wins": pa.array(c[b, s, q, WINS]), "raw_exposures": pa.array(exposures[b, s, q]),
        "raw_completed_exposures": pa.array(c[b, s, q, COMPLETED]), "raw_safety_limit_exposures": pa.array(c[b, s, q, SAFETY]),
    }, schema=pa.schema([pa.field(name, typ, nullable=False) for name, typ in (
        ("root_seed", pa.int64()), ("k", pa.int16()), ("deterministic_batch_id", pa.int32()), ("strategy", pa.int32()), ("seat", pa.int16()),
        ("raw_wins", pa.int64()), ("raw_exposures", pa.int64()), ("raw_completed_exposures", pa.int64()),
        ("raw_safety_limit_exposures", pa.int64()))]))


def _effects(wins, exposures, completed, safety, k: int) -> dict:
    import pyarrow as pa

    chance = np.full(len(wins), 1.0 / k)
    rate = _rate(wins, exposures)
    given = _rate(wins, np.where(completed == 0, 1, completed))
    return {"raw_wins": pa.array(wins), "raw_exposures": pa.array(exposures), "raw_completed_exposures": pa.array(completed),
            "raw_safety_limit_exposures": pa.array(safety), "chance_baseline": pa.array(chance), "win_rate": pa.array(rate),
            "win_rate_per_attempt": pa.array(rate), "win_rate_given_completion": pa.array(given, mask=completed == 0),
            "safety_limit_exposure_rate": pa.array(_rate(safety, exposures)), "raw_losses": pa.array(exposures - wins),
            "seat_effect": pa.array(rate - chance)}


def within_k_frames(counts: SeatCounts, strategy_ids, root_seed: int):
    """``seat_effects.parquet`` (strategy x seat in ascending (ID, seat), cells with an exposure) and
    ``seat_population_effects.parquet`` (per seat) of one player count."""
    import pyarrow as pa

    ids = np.asarray(strategy_ids, dtype=np.int64)
    id_ranks(ids, counts.counts.shape[1])
    k = counts.k
    total = counts.counts.sum(axis=0)[np.argsort(ids, kind="stable")]  # [S][k][3], ascending ID
    exposures = total[..., COMPLETED] + total[..., SAFETY]
    s, q = np.nonzero(exposures)
    n = len(s)
    by_k = pa.table({"root_seed": pa.array(np.full(n, int(root_seed), np.int64)), "k": pa.array(np.full(n, k, np.int16)),
                     "strategy": pa.array(np.sort(ids)[s].astype(np.int32)), "seat": pa.array((q + 1).astype(np.int16)),
                     **_effects(total[s, q, WINS], exposures[s, q], total[s, q, COMPLETED], total[s, q, SAFETY], k)})
    pop = total.sum(axis=0)  # [k][3]
    pop_exposures = pop[:, COMPLETED] + pop[:, SAFETY]
    seats = np.nonzero(pop_exposures)[0]
    population = pa.table({"root_seed": pa.array(np.full(len(seats), int(root_seed), np.int64)), "k": pa.array(np.full(len(seats), k, np.int16)),
                           "seat": pa.array((seats + 1).astype(np.int16)),
                           **_effects(pop[seats, WINS], pop_exposures[seats], pop[seats, COMPLETED], pop[seats, SAFETY], k)})
    return by_k, population


def declared_weights(ks, method: str = "equal-k", k_weights=None) -> dict:
    """``k_aggregation`` -> the weight of every player count (_declared_weights :379-390): a declared mapping must cover exactly
    the configured player counts."""
    ks = [int(k) for k in ks]
    if method == "equal-k":
        return {k: 1.0 / len(ks) for k in ks}
    configured = {int(k): float(w) for k, w in dict(k_weights or {}).items()}
    if set(configured) != set(ks):
        raise ValueError("declared seat standardization weights must cover every configured k")
    return configured


def standardized_frames(by_k: dict, population_by_k: dict, ks, weights: dict):
    """``seat_effects_standardized_across_k.parquet`` and ``seat_exposure_mixture.parquet`` from the per-k frames of
    ``within_k_frames``: strategies and seats every player count supports, then the population rows."""
    import pyarrow as pa

    ks = [int(k) for k in ks]
    cols = ("root_seed", "seat_effect", "raw_wins", "raw_exposures", "raw_completed_exposures", "raw_safety_limit_exposures")

    def cells_of(table, keyed: bool) -> dict:
        data = {name: table.column(name).to_pylist() for name in cols + ("seat",) + (("strategy",) if keyed else ())}
        return {((data["strategy"][i], data["seat"][i]) if keyed else data["seat"][i]): {name: data[name][i] for name in cols}
                for i in range(table.num_rows)}

    strat_cells = {k: cells_of(by_k[k], True) for k in ks}
    pop_cells = {k: cells_of(population_by_k[k], False) for k in ks}
    common = set.intersection(*({key[0] for key in strat_cells[k]} for k in ks))
    std, mix = [], []

    def emit(scope: str, strategy, seat: int, cells: list) -> None:
        effect = sum(float(cell["seat_effect"]) * weights[k] for k, cell in zip(ks, cells))
        wins = sum(int(cell["raw_wins"]) for cell in cells)
        exposures = sum(int(cell["raw_exposures"]) for cell in cells)
        baseline_mass = sum(int(cell["raw_exposures"]) / k for k, cell in zip(ks, cells))
        head = {"root_seed": int(cells[0]["root_seed"]), "effect_scope": scope, "strategy": strategy, "seat": seat, "common_k_support": ks}
        std.append({**head, "standardized_seat_effect": effect})
        mix.append({**head, "raw_wins": wins, "raw_exposures": exposures,
                    "raw_completed_exposures": sum(int(cell["raw_completed_exposures"]) for cell in cells),
                    "raw_safety_limit_exposures": sum(int(cell["raw_safety_limit_exposures"]) for cell in cells),
                    "exposure_weighted_baseline": baseline_mass / exposures,
                    "exposure_weighted_seat_effect": wins / exposures - baseline_mass / exposures})

    seats = range(1, min(ks) + 1)
    for strategy in sorted(common):
        for seat in seats:
            cells = [strat_cells[k].get((strategy, seat)) for k in ks]
            if all(cell is not None for cell in cells):
                emit("strategy", int(strategy), seat, cells)
    for seat in seats:
        cells = [pop_cells[k].get(seat) for k in ks]
        if all(cell is not None for cell in cells):
            emit("population", None, seat, cells)
    head = [("root_seed", pa.int64()), ("effect_scope", pa.string()), ("strategy", pa.int64()), ("seat", pa.int64()),
            ("common_k_support", pa.list_(pa.int64()))]
    std_schema = pa.schema(head + [("standardized_seat_effect", pa.float64())])
    mix_schema = pa.schema(head + [("raw_wins", pa.int64()), ("raw_exposures", pa.int64()), ("raw_completed_exposures", pa.int64()),
                                   ("raw_safety_limit_exposures", pa.int64()), ("exposure_weighted_baseline", pa.float64()),
                                   ("exposure_weighted_seat_effect", pa.float64())])
    return pa.Table.from_pylist(std, schema=std_schema), pa.Table.from_pylist(mix, schema=mix_schema)


def selfplay_frame(by_k: dict):
    """``seat_selfplay_p1.parquet``: games whose seats all hold one strategy.  With unique IDs that is every game of k = 1 (the frame
    is its seat-1 row of ``within_k_frames`` per strategy) and no game of k >= 2."""
    import pyarrow as pa

    rows = []
    for k in sorted(by_k):
        if int(k) != 1:
            continue
        t = by_k[k].to_pydict()
        for i in range(len(t["strategy"])):
            wins, completed, safety = int(t["raw_wins"][i]), int(t["raw_completed_exposures"][i]), int(t["raw_safety_limit_exposures"][i])
            attempted = completed + safety
            rows.append({"root_seed": int(t["root_seed"][i]), "k": 1, "strategy": int(t["strategy"][i]), "p1_wins": wins,
                         "games_attempted": attempted, "games_completed": completed, "games_safety_limit": safety,
                         "p1_win_rate_per_attempt": wins / attempted,
                         "p1_win_rate_given_completion": wins / completed if completed else None,
                         "p1_effect_vs_chance": wins / attempted - 1.0 / 1})
    schema = pa.schema([("root_seed", pa.int64()), ("k", pa.int64()), ("strategy", pa.int64()), ("p1_wins", pa.int64()),
                        ("games_attempted", pa.int64()), ("games_completed", pa.int64()), ("games_safety_limit", pa.int64()),
                        ("p1_win_rate_per_attempt", pa.float64()), ("p1_win_rate_given_completion", pa.float64()),
                        ("p1_effect_vs_chance", pa.float64())])
    if not rows:  # (the reference's frame without rows has columns and no types: Arrow's null type)
        schema = pa.schema([(name, pa.null()) for name in schema.names])
    return pa.Table.from_pylist(rows, schema=schema)


def mirrored_frame(pairs: "MirroredPairs | None", root_seed: int):
    """``seat_mirrored_games.parquet``: one row per strategy pair, the mean as one division, null where nothing paired."""
    import pyarrow as pa

    if pairs is None:  # a run without a two-player count: the reference's frame without rows (columns of Arrow's null type)
        names = ("root_seed", "k", "strategy_a", "strategy_b", "paired_mirrored_games", "games_attempted", "games_completed",
                 "games_safety_limit", "unpaired_forward_games", "unpaired_reverse_games", "mean_p1_win_difference")
        return pa.table({name: pa.nulls(0) for name in names})
    s = pairs.sums
    n = len(s)
    matched = s[:, 0]
    mean = _rate(s[:, 1], np.where(matched == 0, 1, matched))
    return pa.table({
        "root_seed": pa.array(np.full(n, int(root_seed), np.int64)), "k": pa.array(np.full(n, 2, np.int16)),
        "strategy_a": pa.array(pairs.ids[:, 0].astype(np.int32)), "strategy_b": pa.array(pairs.ids[:, 1].astype(np.int32)),
        "paired_mirrored_games": pa.array(matched), "games_attempted": pa.array(s[:, 2] + s[:, 3]), "games_completed": pa.array(s[:, 2]),
        "games_safety_limit": pa.array(s[:, 3]), "unpaired_forward_games": pa.array(s[:, 4]), "unpaired_reverse_games": pa.array(s[:, 5]),
        "mean_p1_win_difference": pa.array(mean, mask=matched == 0)})
