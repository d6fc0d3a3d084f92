"""The rare-event game rows and quantile thresholds of the reference's game-stats stage, without rows.

``analysis/game_stats.py`` lists every game in which at least two seats reach ``analysis.rare_event_target_score`` or which
completed with a runner-up margin ``<=`` one of the margin thresholds (``_build_rare_event_summary_shard`` :2715-2984,
``_rare_event_details`` :2987-3153), and can choose both thresholds as order statistics (``_resolve_rare_event_thresholds``
:3293-3328): the margin threshold as a quantile of the runner-up margins of completed games, the target score as the
``1 - target_rate`` quantile of the SECOND-HIGHEST seat score of every attempted game with at least two seats.

A flagged game is a function of the 16-byte game record of the game-stats pass plus the shuffle's permutation, and both
quantiles are order statistics of integer histograms (scores are multiples of 50), so ``fk_tournament_run_rare_events`` returns

* ``strategy_second [S][B]`` / ``game_second [B]``: histograms of ``second-highest score / 50`` (k >= 2, safety-limit games too);
* the flagged games in ascending (shuffle, game) order — ``event_head uint32 [n][4]`` (shuffle - shuffle_begin; game | completed
  << 16 | multi << 17 | threshold mask << 18; margin / 50; spread / 50) and ``event_seats uint16 [n][k]`` (strategy TABLE indices).

:class:`RareEventSummary` / :func:`events_from_rows` are the same statement in NumPy over engine rows; the frame builders lay the
events out as the reference's two files do."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Mapping, Sequence

import numpy as np

from .game_stats import (ATTEMPTED, COMPLETED, MULTI_TARGET, SCORE_UNIT, STRATEGY_UNIT, GameStatsSummary, _add_padded,
                         _observations_arrow, rare_event_schema, rare_event_summary_table)

DEVICE_SECOND_BINS = 1024   # device window of second / 50 (51 200 points); beyond it: exact spill entries of kind 3
SPILL_SECOND = 3
MAX_THRESHOLDS = 8
DEFAULT_BATCH_GAMES = 65_536  # the scanner batch of _rare_event_details :3051
H_SHUFFLE, H_BITS, H_MARGIN, H_SPREAD = 0, 1, 2, 3
BIT_COMPLETED, BIT_MULTI, BIT_MASK = 16, 17, 18


# ------------------------------------------------------------------------------------------------------------- event records
def event_fields(head: np.ndarray) -> dict:
    """The columns packed in ``event_head``."""
    head = np.asarray(head, dtype=np.uint32).reshape(-1, 4)
    bits = head[:, H_BITS]
    return {"shuffle": head[:, H_SHUFFLE].astype(np.int64), "game": (bits & 0xffff).astype(np.int64),
            "completed": ((bits >> BIT_COMPLETED) & 1).astype(bool), "multi": ((bits >> BIT_MULTI) & 1).astype(bool),
            "mask": ((bits >> BIT_MASK) & 0xff).astype(np.int64), "margin50": head[:, H_MARGIN].astype(np.int64),
            "spread50": head[:, H_SPREAD].astype(np.int64)}


def _check_thresholds(thresholds: Sequence[int]) -> list[int]:
    thr = [int(t) for t in thresholds]
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} margin thresholds per call, got {len(thr)}")
    return thr


def events_from_rows(rows: np.ndarray, k: int, games_per_shuffle: int, rare_target_score: int,
                     thresholds: Sequence[int]) -> tuple[np.ndarray, np.ndarray]:
    """The host statement of the flagged-game list over engine rows (``backend.row_dtype(k)``, in (shuffle, game) order):
    ``(event_head [n][4] uint32, event_seats [n][k] uint16)``."""
    k, gps = int(k), int(games_per_shuffle)
    thr = _check_thresholds(thresholds)
    n = len(rows)
    if n == 0:
        return np.zeros((0, 4), np.uint32), np.zeros((0, k), np.uint16)
    completed = rows["status"] == 0
    scores = rows["seats"]["score"].astype(np.int64).reshape(n, k)
    strat = rows["seats"]["strategy"].astype(np.int64).reshape(n, k)
    srt = np.sort(scores, axis=1)
    margins = completed & (k >= 2)
    runner = np.where(margins, srt[:, -1] - srt[:, -2] if k >= 2 else 0, 0)
    spread = np.where(margins, srt[:, -1] - srt[:, 0], 0)
    multi = (scores >= int(rare_target_score)).sum(axis=1) >= 2
    mask = np.zeros(n, np.int64)
    for i, t in enumerate(thr):
        mask |= (margins & (runner <= t)).astype(np.int64) << i
    keep = np.flatnonzero(multi | (mask != 0))
    ordinal = keep.astype(np.int64)
    head = np.zeros((len(keep), 4), np.uint32)
    head[:, H_SHUFFLE] = ordinal // gps
    head[:, H_BITS] = ((ordinal % gps) | (completed[keep].astype(np.int64) << BIT_COMPLETED) | (multi[keep].astype(np.int64) << BIT_MULTI)
                       | (mask[keep] << BIT_MASK))
    head[:, H_MARGIN] = runner[keep] // SCORE_UNIT
    head[:, H_SPREAD] = spread[keep] // SCORE_UNIT
    return head, strat[keep].astype(np.uint16)


def concat_events(parts: Sequence[tuple[np.ndarray, np.ndarray]], shuffle_offsets: Sequence[int]) -> tuple[np.ndarray, np.ndarray]:
    """The lists of consecutive shuffle ranges as the list of the whole range: part ``i`` began ``shuffle_offsets[i]`` shuffles
    after the first."""
    heads, seats = [], []
    for (h, s), off in zip(parts, shuffle_offsets):
        h = np.array(h, dtype=np.uint32).reshape(-1, 4)
        h[:, H_SHUFFLE] += np.uint32(off)
        heads.append(h)
        s = np.asarray(s, dtype=np.uint16)
        seats.append(s if s.ndim == 2 and len(s) == len(h) else s.reshape(len(h), -1))
    if not heads:
        return np.zeros((0, 4), np.uint32), np.zeros((0, 0), np.uint16)
    return np.concatenate(heads), np.concatenate(seats)


# -------------------------------------------------------------------------------------------------------- sufficient statistics
@dataclass
class RareEventSummary:
    """``GameStatsSummary`` + the second-highest-score histograms of the same range (``second / 50``; empty for k = 1)."""

    stats: GameStatsSummary
    strategy_second: np.ndarray
    game_second: np.ndarray

    @property
    def k(self) -> int:
        return self.stats.k

    @classmethod
    def from_engine(cls, result: dict, k: int) -> "RareEventSummary":
        r = result["rare_events"]
        return cls(GameStatsSummary.from_engine(result, k), np.asarray(r["strategy_second"], np.int64), np.asarray(r["game_second"], np.int64))

    @classmethod
    def from_rows(cls, rows: np.ndarray, k: int, n_strategies: int, rare_target_score: int) -> "RareEventSummary":
        k, S = int(k), int(n_strategies)
        stats = GameStatsSummary.from_rows(rows, k, S, rare_target_score)
        if len(rows) == 0 or k < 2:
            return cls(stats, np.zeros((S, 1), np.int64), np.zeros(1, np.int64))
        scores = rows["seats"]["score"].astype(np.int64).reshape(len(rows), k)
        strat = rows["seats"]["strategy"].astype(np.int64).reshape(len(rows), k)
        second = np.sort(scores, axis=1)[:, -2] // SCORE_UNIT
        B = int(second.max()) + 1
        game = np.bincount(second, minlength=B).astype(np.int64)
        per = np.bincount(strat.reshape(-1) * B + np.repeat(second, k), minlength=S * B).reshape(S, B).astype(np.int64)
        return cls(stats, per, game)

    def merge(self, other: "RareEventSummary") -> "RareEventSummary":
        return RareEventSummary(self.stats.merge(other.stats), _add_padded(self.strategy_second, other.strategy_second),
                                _add_padded(self.game_second, other.game_second))

    def multi_tail(self, target_score: int) -> tuple[np.ndarray, int]:
        """(per strategy exposure, per game) counts with ``second >= target_score``: exactly the games where at least two seats
        reach it."""
        first = max(int(math.ceil(int(target_score) / SCORE_UNIT)), 0)
        return self.strategy_second[:, first:].sum(axis=1), int(self.game_second[first:].sum())

    def under_target(self, target_score: int) -> GameStatsSummary:
        """The game statistics with the multi-target counts of ``target_score`` instead of the launch's own rare target."""
        s = self.stats
        per, game = self.multi_tail(target_score)
        counts, g = s.strategy_counts.copy(), s.game_counts.copy()
        counts[:, MULTI_TARGET] = per
        g[MULTI_TARGET] = game
        return GameStatsSummary(s.k, counts, s.strategy_rounds, s.strategy_runner, s.strategy_spread, g, s.game_rounds, s.game_runner)


def merge_second_spills(strategy_second: np.ndarray, game_second: np.ndarray, spill: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Add the spill entries of kind 3 ``(strategy index or -1, 3, second / 50)`` into histograms widened to hold them."""
    spill = np.asarray(spill, dtype=np.int64).reshape(-1, 3)
    spill = spill[spill[:, 1] == SPILL_SECOND]
    if len(spill) == 0:
        return strategy_second, game_second
    S = strategy_second.shape[0]
    if np.any(spill[:, 2] < 0) or np.any(spill[:, 0] >= S) or np.any(spill[:, 0] < -1):
        raise ValueError("malformed second-score spill entry")
    width = max(int(spill[:, 2].max()) + 1, strategy_second.shape[1], game_second.shape[0])
    per = _add_padded(strategy_second, np.zeros((S, width), np.int64))
    game = _add_padded(game_second, np.zeros(width, np.int64))
    g = spill[spill[:, 0] < 0]
    np.add.at(game, g[:, 2], 1)
    s = spill[spill[:, 0] >= 0]
    np.add.at(per, (s[:, 0], s[:, 2]), 1)
    return per, game


# ---------------------------------------------------------------------------------------------------------------- thresholds
def _quantile_from_hist(hist50: np.ndarray, quantile: float) -> int | None:
    """``_quantile_from_counts`` (:3422-3439) over a histogram of ``value / 50``: the value in points."""
    h = np.asarray(hist50, dtype=np.int64)
    total = int(h.sum())
    if total <= 0:
        return None
    values = np.flatnonzero(h)
    if quantile <= 0.0:
        return int(values[0]) * SCORE_UNIT
    if quantile >= 1.0:
        return int(values[-1]) * SCORE_UNIT
    cutoff = int(math.ceil(total * quantile))
    running = 0
    for v in values:
        running += int(h[v])
        if running >= cutoff:
            return int(v) * SCORE_UNIT
    return int(values[-1]) * SCORE_UNIT


def resolve_rare_event_thresholds(summaries_by_k: Mapping[int, RareEventSummary], thresholds: Sequence[int], target_score: int,
                                  margin_quantile: float | None, target_rate: float | None) -> tuple[tuple[int, ...], int]:
    """``_resolve_rare_event_thresholds`` (:3293-3328) from the histograms pooled over every player count: the margin histogram
    is ``game_runner`` (completed games), the target histogram ``game_second`` with quantile ``1 - target_rate``.  An empty
    histogram leaves the configured value; a resolved margin quantile replaces the whole threshold tuple by one value."""
    resolved = tuple(int(t) for t in thresholds)
    target = int(target_score)
    if margin_quantile is None and target_rate is None:
        return resolved, target
    if margin_quantile is not None and not 0.0 < margin_quantile < 1.0:
        raise ValueError("rare_event_margin_quantile must be between 0 and 1")
    if target_rate is not None and not 0.0 < target_rate < 1.0:
        raise ValueError("rare_event_target_rate must be between 0 and 1")
    if margin_quantile is not None:
        pooled = np.zeros(1, np.int64)
        for s in summaries_by_k.values():
            pooled = _add_padded(pooled, np.asarray(s.stats.game_runner, np.int64))
        value = _quantile_from_hist(pooled, margin_quantile)
        if value is not None:
            resolved = (value,)
    if target_rate is not None:
        pooled = np.zeros(1, np.int64)
        for s in summaries_by_k.values():
            pooled = _add_padded(pooled, np.asarray(s.game_second, np.int64))
        value = _quantile_from_hist(pooled, 1.0 - target_rate)
        if value is not None:
            target = value
    return resolved, target


# -------------------------------------------------------------------------------------------------------------------- frames
def _batch_bounds(batch_games, n_games: int) -> np.ndarray:
    """Ends of the reader's batches over the k's ``n_games`` curated rows: a fixed length or the lengths themselves."""
    if isinstance(batch_games, (int, np.integer)):
        size = int(batch_games)
        if size < 1:
            raise ValueError("batch length must be >= 1")
        return np.minimum(np.arange(1, (n_games + size - 1) // size + 1, dtype=np.int64) * size, n_games)
    ends = np.cumsum(np.asarray(list(batch_games), dtype=np.int64))
    if len(ends) == 0 or int(ends[-1]) != int(n_games) or np.any(np.diff(np.concatenate([[0], ends])) < 0):
        raise ValueError("batch lengths must cover the player count's games exactly")
    return ends


def rare_event_game_table(head: np.ndarray, seats: np.ndarray, k: int, games_per_shuffle: int, n_games: int,
                          strategy_ids: Sequence[int], thresholds: Sequence[int], *, details: bool, batch_games=DEFAULT_BATCH_GAMES,
                          strategy_arrow=None):
    """The per-game rows of one player count in the reference's schema and order: per read batch the flagged games SEAT-MAJOR
    (every ``P1`` strategy of the batch's flagged games, then ``P2`` ...: ``melt``, :2893-2905).  ``details``: the
    ``rare_events_details.parquet`` form (flags and observation columns uint8); otherwise the summary-shard form (flags float64,
    observations uint8).  ``batch_games``: the reader's batch length or its batch lengths in games."""
    import pyarrow as pa

    strategy_arrow = strategy_arrow if strategy_arrow is not None else pa.int32()
    thr = _check_thresholds(thresholds)
    f = event_fields(head)
    seats = np.asarray(seats, dtype=np.int64).reshape(len(f["shuffle"]), int(k))
    ids = np.asarray(strategy_ids, dtype=np.int64)
    ordinal = f["shuffle"] * int(games_per_shuffle) + f["game"]
    if np.any(np.diff(ordinal) <= 0) or (len(ordinal) and int(ordinal[-1]) >= int(n_games)):
        raise ValueError("events must be in ascending (shuffle, game) order inside the range")
    ends = _batch_bounds(batch_games, int(n_games))
    batch_of = np.searchsorted(ends, ordinal, side="right")
    # seat-major inside a batch: sort (batch, seat, event)
    n, k = len(ordinal), int(k)
    ev = np.tile(np.arange(n, dtype=np.int64), k)
    seat = np.repeat(np.arange(k, dtype=np.int64), n)
    order = np.lexsort((ev, seat, batch_of[ev]))
    ev, seat = ev[order], seat[order]
    flag_np = np.uint8 if details else np.float64
    flag_arrow = pa.uint8() if details else pa.float64()
    schema = rare_event_schema(thr, strategy_arrow, pa.uint8())
    schema = pa.schema([fld.with_type(flag_arrow) if fld.name == "multi_reached_target" or fld.name.startswith("margin_le_") else fld
                        for fld in schema])
    completed = f["completed"][ev]
    valid = completed & (k >= 2)
    data = {
        "summary_level": np.full(len(ev), "game", dtype=object),
        "observational_unit": np.full(len(ev), STRATEGY_UNIT, dtype=object),
        "strategy": ids[seats[ev, seat]] if len(ev) else np.zeros(0, np.int64),
        "n_players": np.full(len(ev), k, dtype=np.int32),
        "termination_status": np.where(completed, "completed", "safety_limit").astype(object),
        "margin_runner_up": np.where(valid, (f["margin50"][ev] * SCORE_UNIT).astype(np.float64), np.nan),
        "score_spread": np.where(valid, (f["spread50"][ev] * SCORE_UNIT).astype(np.float64), np.nan),
        "multi_reached_target": f["multi"][ev].astype(flag_np),
        "observations": np.ones(len(ev), dtype=np.uint8),
        "completed_observations": completed.astype(np.uint8),
        "safety_limit_observations": (~completed).astype(np.uint8),
    }
    for i, t in enumerate(thr):
        data[f"margin_le_{t}"] = ((f["mask"][ev] >> i) & 1).astype(flag_np)
    data["strategy"] = pa.array(data["strategy"], type=pa.int64()).cast(strategy_arrow)
    return pa.Table.from_pydict(data, schema=schema)


def rare_events_table(events_by_k: Mapping[int, tuple], summaries_by_k: Mapping[int, RareEventSummary], strategy_ids: Sequence[int],
                      thresholds: Sequence[int], target_score: int, *, batch_games=DEFAULT_BATCH_GAMES, strategy_arrow=None):
    """``rare_events.parquet`` (``_rare_event_flags`` :2272-2400): the game rows of every player count in ascending k, cast to
    the final schema, then the summary rows under the same thresholds and target.  ``events_by_k[k] = (head, seats,
    games_per_shuffle, n_games)``; ``batch_games``: one value or a mapping by k.  ``None`` when no game is flagged."""
    import pyarrow as pa

    strategy_arrow = strategy_arrow if strategy_arrow is not None else pa.int32()
    under = {int(k): s.under_target(target_score) for k, s in summaries_by_k.items()}
    summary = rare_event_summary_table(under, strategy_ids, thresholds, strategy_arrow=strategy_arrow)
    if summary is None:
        return None
    parts = []
    for k in sorted(events_by_k):
        head, seats, gps, n_games = events_by_k[k]
        bg = batch_games[k] if isinstance(batch_games, Mapping) else batch_games
        t = rare_event_game_table(head, seats, k, gps, n_games, strategy_ids, thresholds, details=False, batch_games=bg,
                                  strategy_arrow=strategy_arrow)
        parts.append(t if t.schema.equals(summary.schema) else t.cast(summary.schema, safe=False))
    return pa.concat_tables(parts + [summary])


def rare_event_details_table(events_by_k: Mapping[int, tuple], strategy_ids: Sequence[int], thresholds: Sequence[int], *,
                             batch_games=DEFAULT_BATCH_GAMES, strategy_arrow=None):
    """``rare_events_details.parquet`` (``_rare_event_details`` :2987-3153): the details rows of every player count in
    ascending k; ``None`` when there is none (the reference then leaves no file)."""
    import pyarrow as pa

    parts = []
    for k in sorted(events_by_k):
        head, seats, gps, n_games = events_by_k[k]
        bg = batch_games[k] if isinstance(batch_games, Mapping) else batch_games
        parts.append(rare_event_game_table(head, seats, k, gps, n_games, strategy_ids, thresholds, details=True, batch_games=bg,
                                           strategy_arrow=strategy_arrow))
    table = pa.concat_tables(parts) if parts else None
    return table if table is not None and table.num_rows else None


def tail_equals_multi_target(summary: RareEventSummary, rare_target_score: int) -> bool:
    """The invariant of the launch's own rare target: the tail of the second-score histograms equals its MULTI_TARGET counts."""
    per, game = summary.multi_tail(rare_target_score)
    return bool(np.array_equal(per, summary.stats.strategy_counts[:, MULTI_TARGET]) and game == int(summary.stats.game_counts[MULTI_TARGET]))


__all__ = ["RareEventSummary", "events_from_rows", "concat_events", "event_fields", "merge_second_spills",
           "resolve_rare_event_thresholds", "rare_event_game_table", "rare_events_table", "rare_event_details_table",
           "tail_equals_multi_target", "ATTEMPTED", "COMPLETED"]
