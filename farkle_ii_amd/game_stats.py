"""The reference's game-stats stage per player count, from exact histograms instead of rows.

``analysis/game_stats.py`` (``_compute_k_game_stats`` :840-1220) reads every curated row of a (root, k) and keeps, per strategy over
its seat exposures and per player count over its games, an ``_UnweightedAccumulator`` of ``n_rounds`` (exact histogram + float
``total`` / ``total_sq``) and, over COMPLETED games with at least two valid scores, ``_BinnedAccumulator``\\ s of the runner-up margin
``max - second max`` and the score spread ``max - min`` of the game's seat scores (25-point bins, :3378-3406).  The rare-event
summary rows of ``_rare_event_flags`` (:2272-2400) are sums of the same games: observations, completed, safety-limit, games where at
least two seats reach ``analysis.rare_event_target_score``, and completed games with ``margin_runner_up <= thr``.

Seat scores are multiples of 50 and ``n_rounds`` is an integer, so one set of integer histograms holds all of it
(``fk_tournament_run_game_stats``; :meth:`GameStatsSummary.from_rows` is the same statement in NumPy).  The reference's floats
are then reproduced bit for bit: its float sums of integers are exact while every partial sum stays below 2**53, which
:func:`_exact_float` checks instead of emitting different bits."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Mapping, Sequence

import numpy as np

DEFAULT_MARGIN_THRESHOLDS = (500, 1000)  # analysis.game_stats_margin_thresholds (reference config.py:323)
DEFAULT_RARE_TARGET_SCORE = 10_000       # analysis.rare_event_target_score (config.py:325)
MARGIN_BIN_WIDTH = 25.0                  # _MARGIN_BIN_WIDTH
SCORE_UNIT = 50                          # margins are kept in units of 50 points
STRATEGY_UNIT = "seated_strategy_exposure_per_attempted_game"  # _ATTEMPTED_STRATEGY_UNIT
GAME_UNIT = "attempted_game"                                   # _ATTEMPTED_GAME_UNIT
# count columns of GameStatsSummary.strategy_counts / game_counts (fk_tournament_run_game_stats)
ATTEMPTED, COMPLETED, SAFETY, MULTI_TARGET = 0, 1, 2, 3
# device histogram windows (values beyond them come back as exact spill entries)
DEVICE_ROUNDS_BINS, DEVICE_MARGIN_BINS = 1024, 512
EXACT_LIMIT = 2 ** 53


def _add_padded(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """``a + b`` for histograms whose last axis may differ in length (the shorter one is zero beyond its end)."""
    n = max(a.shape[-1], b.shape[-1])
    out = np.zeros(a.shape[:-1] + (n,), dtype=np.int64)
    out[..., :a.shape[-1]] += a
    out[..., :b.shape[-1]] += b
    return out


@dataclass
class GameStatsSummary:
    """The exact sufficient statistics of one (root, k) range.  Strategies are TABLE indices; margins are in units of 50 points.

    ``strategy_counts [S][4]`` / ``game_counts [4]``: attempted, completed, safety-limit, multi-target games (``ATTEMPTED`` ...);
    ``strategy_rounds [S][R]`` / ``game_rounds [R]``: ``n_rounds`` histograms; ``strategy_runner`` / ``strategy_spread [S][M]`` and
    ``game_runner [M]``: histograms of ``margin / 50`` over completed games with ``k >= 2``."""

    k: int
    strategy_counts: np.ndarray
    strategy_rounds: np.ndarray
    strategy_runner: np.ndarray
    strategy_spread: np.ndarray
    game_counts: np.ndarray
    game_rounds: np.ndarray
    game_runner: np.ndarray

    @property
    def n_strategies(self) -> int:
        return int(self.strategy_counts.shape[0])

    @classmethod
    def from_engine(cls, result: dict, k: int) -> "GameStatsSummary":
        """From ``Engine.tournament_game_stats(...)["game_stats"]`` (spills already merged)."""
        g = result["game_stats"] if "game_stats" in result else result
        return cls(int(k), *(np.asarray(g[name], dtype=np.int64) for name in (
            "strategy_counts", "strategy_rounds", "strategy_runner", "strategy_spread", "game_counts", "game_rounds", "game_runner")))

    @classmethod
    def empty(cls, k: int, n_strategies: int) -> "GameStatsSummary":
        z = np.zeros
        return cls(int(k), z((n_strategies, 4), np.int64), z((n_strategies, 1), np.int64), z((n_strategies, 1), np.int64),
                   z((n_strategies, 1), np.int64), z(4, np.int64), z(1, np.int64), z(1, np.int64))

    @classmethod
    def from_rows(cls, rows: np.ndarray, k: int, n_strategies: int, rare_target_score: int = DEFAULT_RARE_TARGET_SCORE) -> "GameStatsSummary":
        """The host statement over engine rows (``backend.row_dtype(k)``: status 0 = completed, seat ``strategy`` = table index,
        ``score`` in points)."""
        k = int(k)
        S = int(n_strategies)
        if len(rows) == 0:
            return cls.empty(k, S)
        rounds = rows["n_rounds"].astype(np.int64)
        completed = rows["status"] == 0
        scores = rows["seats"]["score"].astype(np.int64).reshape(len(rows), k)
        strat = rows["seats"]["strategy"].astype(np.int64).reshape(len(rows), k)
        if np.any(scores % SCORE_UNIT):
            raise ValueError("seat scores must be multiples of 50")
        srt = np.sort(scores, axis=1)
        margins = completed & (k >= 2)
        runner = (srt[:, -1] - srt[:, -2]) // SCORE_UNIT if k >= 2 else np.zeros(len(rows), np.int64)
        spread = (srt[:, -1] - srt[:, 0]) // SCORE_UNIT
        multi = (scores >= int(rare_target_score)).sum(axis=1) >= 2
        R = int(rounds.max()) + 1
        M = int(max(runner[margins].max(initial=0), spread[margins].max(initial=0))) + 1

        game_counts = np.array([len(rows), completed.sum(), (~completed).sum(), multi.sum()], dtype=np.int64)
        game_rounds = np.bincount(rounds, minlength=R).astype(np.int64)
        game_runner = np.bincount(runner[margins], minlength=M).astype(np.int64)
        # one exposure per (game, seat)
        s = strat.reshape(-1)
        rep = lambda a: np.repeat(a, k)  # noqa: E731
        e_rounds, e_comp, e_multi, e_marg = rep(rounds), rep(completed), rep(multi), rep(margins)
        counts = np.zeros((S, 4), dtype=np.int64)
        counts[:, ATTEMPTED] = np.bincount(s, minlength=S)
        counts[:, COMPLETED] = np.bincount(s[e_comp], minlength=S)
        counts[:, SAFETY] = np.bincount(s[~e_comp], minlength=S)
        counts[:, MULTI_TARGET] = np.bincount(s[e_multi], minlength=S)
        s_rounds = np.bincount(s * R + e_rounds, minlength=S * R).reshape(S, R).astype(np.int64)
        sm = s[e_marg]
        s_runner = np.bincount(sm * M + rep(runner)[e_marg], minlength=S * M).reshape(S, M).astype(np.int64)
        s_spread = np.bincount(sm * M + rep(spread)[e_marg], minlength=S * M).reshape(S, M).astype(np.int64)
        return cls(k, counts, s_rounds, s_runner, s_spread, game_counts, game_rounds, game_runner)

    def merge(self, other: "GameStatsSummary") -> "GameStatsSummary":
        """Pure int64 addition: launch groups and ranks combine in any order."""
        if other.k != self.k or other.n_strategies != self.n_strategies:
            raise ValueError("game-stat summaries of different (k, table) do not merge")
        return GameStatsSummary(self.k, self.strategy_counts + other.strategy_counts,
                                _add_padded(self.strategy_rounds, other.strategy_rounds),
                                _add_padded(self.strategy_runner, other.strategy_runner),
                                _add_padded(self.strategy_spread, other.strategy_spread),
                                self.game_counts + other.game_counts, _add_padded(self.game_rounds, other.game_rounds),
                                _add_padded(self.game_runner, other.game_runner))

    def to_arrays(self) -> dict:
        return {"k": self.k, "strategy_counts": self.strategy_counts, "strategy_rounds": self.strategy_rounds,
                "strategy_runner": self.strategy_runner, "strategy_spread": self.strategy_spread, "game_counts": self.game_counts,
                "game_rounds": self.game_rounds, "game_runner": self.game_runner}

    @classmethod
    def from_sums_table(cls, table, strategy_ids: Sequence[int], k: int) -> "GameStatsSummary":
        """The inverse of :meth:`sums_table` for the table whose strategies are ``strategy_ids``."""
        ids = np.asarray(strategy_ids, dtype=np.int64)
        index = {int(v): i for i, v in enumerate(ids)}
        cols = table.to_pydict()
        hist_names = ("n_rounds_hist", "margin_runner_up_hist_50", "score_spread_hist_50")
        width = [max([len(h) for h in cols[name]] + [1]) for name in hist_names]
        out = cls(int(k), np.zeros((len(ids), 4), np.int64), np.zeros((len(ids), width[0]), np.int64),
                  np.zeros((len(ids), width[1]), np.int64), np.zeros((len(ids), width[2]), np.int64), np.zeros(4, np.int64),
                  np.zeros(width[0], np.int64), np.zeros(width[1], np.int64))
        for r, level in enumerate(cols["summary_level"]):
            c = [cols[name][r] for name in ("observations", "completed_observations", "safety_limit_observations", "multi_reached_target")]
            h = [np.asarray(cols[name][r], dtype=np.int64) for name in hist_names]
            if level == "n_players":
                out.game_counts[:] = c
                out.game_rounds[:len(h[0])] = h[0]
                out.game_runner[:len(h[1])] = h[1]
            else:
                i = index[int(cols["strategy"][r])]
                out.strategy_counts[i] = c
                out.strategy_rounds[i, :len(h[0])] = h[0]
                out.strategy_runner[i, :len(h[1])] = h[1]
                out.strategy_spread[i, :len(h[2])] = h[2]
        return out

    def sums_table(self, strategy_ids: Sequence[int]):
        """The raw sufficient statistics as one Arrow table (``<n>p_game_stats_sums.parquet``): one row per strategy that has
        exposures, by ascending ID, then the game-level row (``strategy`` null); histograms are list columns, margins in units of 50."""
        import pyarrow as pa

        ids = np.asarray(strategy_ids, dtype=np.int64)
        order = [int(i) for i in np.argsort(ids, kind="stable") if self.strategy_counts[i, ATTEMPTED] > 0]

        def trim(h: np.ndarray) -> list[int]:
            nz = np.flatnonzero(h)
            return [int(v) for v in h[:nz[-1] + 1]] if len(nz) else []

        rows = [(int(ids[i]), self.strategy_counts[i], self.strategy_rounds[i], self.strategy_runner[i], self.strategy_spread[i])
                for i in order]
        rows.append((None, self.game_counts, self.game_rounds, self.game_runner, np.zeros(0, np.int64)))
        return pa.table({
            "summary_level": pa.array(["strategy"] * len(order) + ["n_players"], pa.string()),
            "strategy": pa.array([r[0] for r in rows], pa.int64()),
            "n_players": pa.array([self.k] * len(rows), pa.int32()),
            "observations": pa.array([int(r[1][ATTEMPTED]) for r in rows], pa.int64()),
            "completed_observations": pa.array([int(r[1][COMPLETED]) for r in rows], pa.int64()),
            "safety_limit_observations": pa.array([int(r[1][SAFETY]) for r in rows], pa.int64()),
            "multi_reached_target": pa.array([int(r[1][MULTI_TARGET]) for r in rows], pa.int64()),
            "n_rounds_hist": pa.array([trim(r[2]) for r in rows], pa.list_(pa.int64())),
            "margin_runner_up_hist_50": pa.array([trim(r[3]) for r in rows], pa.list_(pa.int64())),
            "score_spread_hist_50": pa.array([trim(r[4]) for r in rows], pa.list_(pa.int64())),
        })


def merge_spills(game_stats: dict, spill: np.ndarray, rounds_bins_total: int) -> dict:
    """Add the device's spill entries ``(strategy index or -1, kind, value)`` into histograms widened to hold them; the rounds
    histograms are ``rounds_bins_total`` (= R + 1) wide."""
    out = dict(game_stats)
    spill = np.asarray(spill, dtype=np.int64).reshape(-1, 3)
    S = out["strategy_counts"].shape[0]
    m_need = int(spill[spill[:, 1] != 0, 2].max(initial=-1)) + 1
    r_need = max(int(rounds_bins_total), int(spill[spill[:, 1] == 0, 2].max(initial=-1)) + 1)
    for name, width in (("strategy_rounds", r_need), ("game_rounds", r_need), ("strategy_runner", m_need), ("strategy_spread", m_need),
                        ("game_runner", m_need)):
        a = out[name]
        if a.shape[-1] < width:
            out[name] = _add_padded(a, np.zeros(a.shape[:-1] + (width,), np.int64))
    targets = {(0, True): "strategy_rounds", (1, True): "strategy_runner", (2, True): "strategy_spread", (0, False): "game_rounds",
               (1, False): "game_runner"}
    for who, kind, value in spill:
        name = targets.get((int(kind), int(who) >= 0))
        if name is None or int(who) >= S or value < 0:
            raise ValueError(f"malformed game-stat spill entry {(int(who), int(kind), int(value))}")
        if int(who) >= 0:
            out[name][int(who), int(value)] += 1
        else:
            out[name][int(value)] += 1
    return out


# ------------------------------------------------------------------------------------------------------ the reference's floats
def _exact_float(value: int, what: str) -> float:
    """``float`` of an integer sum, which equals the reference's float64 running sum only below 2**53."""
    if abs(int(value)) > EXACT_LIMIT:
        raise OverflowError(f"game statistics: {what} = {int(value)} exceeds 2**53; the reference's float64 sum is no longer exact "
                            "and its bits cannot be reproduced")
    return float(int(value))


class _Hist:
    """One exact histogram ``counts[v]`` of values ``v * scale`` (scale 1 for n_rounds, 50 for margins)."""

    def __init__(self, counts: np.ndarray, scale: int, what: str):
        c = np.asarray(counts, dtype=np.int64)
        self.values = np.flatnonzero(c)
        self.freq = c[self.values]
        self.scale = int(scale)
        self.count = int(self.freq.sum())
        v = [int(x) * self.scale for x in self.values]
        f = [int(x) for x in self.freq]
        self.total = _exact_float(sum(a * b for a, b in zip(v, f)), f"sum of {what}")
        self.total_sq = _exact_float(sum(a * a * b for a, b in zip(v, f)), f"sum of squared {what}")
        self.points = v
        self.cum = np.cumsum(self.freq)

    def value_at_rank(self, rank: int) -> float:  # _hist_value_at_rank
        i = int(np.searchsorted(self.cum, rank, side="right"))
        return float(self.points[min(i, len(self.points) - 1)])

    # --- _UnweightedAccumulator (exact values)
    def mean_std(self) -> tuple[float, float]:  # _mean_std_from_unweighted: mean**2 form
        if self.count <= 0:
            return float("nan"), float("nan")
        mean = self.total / self.count
        variance = max((self.total_sq / self.count) - (mean ** 2), 0.0)
        return float(mean), float(math.sqrt(variance))

    def quantile_linear(self, q: float) -> float:  # _quantile_linear_from_hist
        if self.count <= 0:
            return float("nan")
        h = (self.count - 1) * q
        lo, hi = int(math.floor(h)), int(math.ceil(h))
        lower, upper = self.value_at_rank(lo), self.value_at_rank(hi)
        return float(lower + (h - lo) * (upper - lower))

    def prob_le(self, thr: float) -> float:  # _probability_le_from_hist
        matched = sum(int(f) for v, f in zip(self.points, self.freq) if v <= thr)
        return float(matched / self.count) if self.count > 0 else float("nan")

    def prob_ge(self, thr: float) -> float:  # _probability_ge_from_hist
        matched = sum(int(f) for v, f in zip(self.points, self.freq) if v >= thr)
        return float(matched / self.count) if self.count > 0 else float("nan")

    # --- _BinnedAccumulator (25-point bins of the same values)
    def bin_ids(self) -> list[int]:
        return [int(math.floor(v / MARGIN_BIN_WIDTH)) for v in self.points]

    def binned_mean_std(self) -> tuple[float, float]:  # _mean_std_from_binned: mean * mean form
        if self.count <= 0:
            return float("nan"), float("nan")
        mean = self.total / self.count
        variance = max((self.total_sq / self.count) - (mean * mean), 0.0)
        return float(mean), float(math.sqrt(variance))

    def binned_quantile(self, q: float) -> float:  # _quantile_from_binned
        if self.count <= 0:
            return float("nan")
        cutoff = int(math.ceil(self.count * q))
        running = 0
        for b, f in zip(self.bin_ids(), self.freq):
            running += int(f)
            if running >= cutoff:
                return float((b + 0.5) * MARGIN_BIN_WIDTH)
        return float(self.points[-1])

    def binned_prob_le(self, thr: float) -> float:  # _probability_le_from_binned
        if self.count <= 0 or not math.isfinite(thr):
            return float("nan")
        tb = int(math.floor(thr / MARGIN_BIN_WIDTH))
        le = sum(int(f) for b, f in zip(self.bin_ids(), self.freq) if b <= tb)
        return float(le / self.count)


def _round_fields(h: _Hist) -> dict:
    mean, std = h.mean_std()
    return {"mean_rounds": mean, "median_rounds": h.quantile_linear(0.5), "std_rounds": std, "p10_rounds": h.quantile_linear(0.1),
            "p50_rounds": h.quantile_linear(0.5), "p90_rounds": h.quantile_linear(0.9), "prob_rounds_le_5": h.prob_le(5),
            "prob_rounds_le_10": h.prob_le(10), "prob_rounds_ge_20": h.prob_ge(20)}


def game_stats_rows(summary: GameStatsSummary, strategy_ids: Sequence[int], k: int,
                    thresholds: Sequence[int] = DEFAULT_MARGIN_THRESHOLDS) -> list[dict]:
    """The list of dicts ``_compute_k_game_stats`` builds (:1077-1184), key order included.  Row order: strategy rows by ascending
    strategy ID, then the ``n_players`` row (the reference's is first encounter in its byte-sized batches)."""
    ids = np.asarray(strategy_ids, dtype=np.int64)
    if len(ids) != summary.n_strategies:
        raise ValueError("strategy_ids must name every strategy of the table")
    rows: list[dict] = []
    for i in np.argsort(ids, kind="stable"):
        c = summary.strategy_counts[i]
        attempted, completed, safety = int(c[ATTEMPTED]), int(c[COMPLETED]), int(c[SAFETY])
        if attempted <= 0:
            continue
        rounds = _Hist(summary.strategy_rounds[i], 1, "n_rounds")
        if attempted != rounds.count or attempted != completed + safety:
            raise ValueError("strategy game-stat exposure conservation failed")
        row = {"summary_level": "strategy", "observational_unit": STRATEGY_UNIT, "strategy": int(ids[i]), "n_players": int(k),
               "observations": attempted, "completed_observations": completed, "safety_limit_observations": safety,
               "safety_limit_observation_rate": safety / attempted}
        row.update(_round_fields(rounds))
        runner = _Hist(summary.strategy_runner[i], SCORE_UNIT, "margin_runner_up")
        spread = _Hist(summary.strategy_spread[i], SCORE_UNIT, "score_spread")
        if runner.count > 0 and spread.count > 0:
            mean_r, std_r = runner.binned_mean_std()
            mean_s, std_s = spread.binned_mean_std()
            row.update({"margin_observations": runner.count, "mean_margin_runner_up": mean_r,
                        "median_margin_runner_up": runner.binned_quantile(0.5), "std_margin_runner_up": std_r,
                        "mean_score_spread": mean_s, "median_score_spread": spread.binned_quantile(0.5), "std_score_spread": std_s})
            for thr in thresholds:
                row[f"prob_margin_runner_up_le_{thr}"] = runner.binned_prob_le(float(thr))
                row[f"prob_score_spread_le_{thr}"] = spread.binned_prob_le(float(thr))
        rows.append(row)
    g = summary.game_counts
    rounds = _Hist(summary.game_rounds, 1, "n_rounds")
    if rounds.count > 0:
        import pandas as pd

        row = {"summary_level": "n_players", "observational_unit": GAME_UNIT, "strategy": pd.NA, "n_players": int(k),
               "observations": rounds.count, "completed_observations": int(g[COMPLETED]), "safety_limit_observations": int(g[SAFETY]),
               "safety_limit_observation_rate": int(g[SAFETY]) / rounds.count}
        row.update(_round_fields(rounds))
        rows.append(row)
    return rows


def game_stats_table(summary: GameStatsSummary, strategy_ids: Sequence[int], k: int,
                     thresholds: Sequence[int] = DEFAULT_MARGIN_THRESHOLDS):
    """The reference's per-k frame as ``pa.Table.from_pandas(frame, preserve_index=False)``; ``None`` when it has no row (the
    reference then writes nothing)."""
    import pandas as pd
    import pyarrow as pa

    rows = game_stats_rows(summary, strategy_ids, k, thresholds)
    if not rows:
        return None
    return pa.Table.from_pandas(pd.DataFrame(rows), preserve_index=False)


def _margin_le(hist50: np.ndarray, thr: int) -> int:
    """Completed games (or exposures) with ``margin_runner_up <= thr`` from a histogram of ``margin / 50``."""
    h = np.asarray(hist50, dtype=np.int64)
    top = int(math.floor(thr / SCORE_UNIT)) if thr >= 0 else -1
    return int(h[:max(min(top + 1, len(h)), 0)].sum())


def rare_event_schema(thresholds: Sequence[int], strategy_arrow, observations_arrow):
    """``_rare_event_schema`` (:2629-2661) with float64 flag columns."""
    import pyarrow as pa

    return pa.schema([
        pa.field("summary_level", pa.string()), pa.field("observational_unit", pa.string()), pa.field("strategy", strategy_arrow),
        pa.field("n_players", pa.int32()), pa.field("termination_status", pa.string()), pa.field("margin_runner_up", pa.float64()),
        pa.field("score_spread", pa.float64()), pa.field("multi_reached_target", pa.float64()),
        pa.field("observations", observations_arrow), pa.field("completed_observations", observations_arrow),
        pa.field("safety_limit_observations", observations_arrow),
        *[pa.field(f"margin_le_{thr}", pa.float64()) for thr in thresholds]])


def _observations_arrow(max_value: int):
    """``_select_int_dtype`` (:3442)."""
    import pyarrow as pa

    if max_value <= 255:
        return pa.uint8()
    if max_value <= 2 ** 31 - 1:
        return pa.int32()
    return pa.int64()


def rare_event_summary_table(summaries_by_k: Mapping[int, GameStatsSummary], strategy_ids: Sequence[int],
                             thresholds: Sequence[int] = DEFAULT_MARGIN_THRESHOLDS, strategy_arrow=None):
    """The summary rows ``_rare_event_flags`` appends to ``rare_events.parquet`` (:2321-2397): per (strategy, k) by ascending
    (strategy ID, k), then per k; ``None`` when no game of the root is flagged (the reference then writes no file).  The
    observation columns' integer type comes from the largest count over every player count: the table is root-level."""
    import pandas as pd
    import pyarrow as pa

    strategy_arrow = strategy_arrow if strategy_arrow is not None else pa.int32()
    ids = np.asarray(strategy_ids, dtype=np.int64)
    thresholds = [int(t) for t in thresholds]
    flagged = 0
    strategy_sums: dict[tuple[int, int], list[int]] = {}
    global_sums: dict[int, list[int]] = {}
    for k, s in summaries_by_k.items():
        k = int(k)
        g = s.game_counts
        game_le = [_margin_le(s.game_runner, t) for t in thresholds]
        flagged += int(g[MULTI_TARGET]) + sum(game_le)
        if int(g[ATTEMPTED]) > 0:
            global_sums[k] = [int(g[ATTEMPTED]), int(g[COMPLETED]), int(g[SAFETY]), int(g[MULTI_TARGET]), *game_le]
        for i in range(s.n_strategies):
            c = s.strategy_counts[i]
            if int(c[ATTEMPTED]) > 0:
                strategy_sums[(int(ids[i]), k)] = [int(c[ATTEMPTED]), int(c[COMPLETED]), int(c[SAFETY]), int(c[MULTI_TARGET]),
                                                   *[_margin_le(s.strategy_runner[i], t) for t in thresholds]]
    if flagged == 0:
        return None
    max_obs = max([v[0] for v in strategy_sums.values()] + [v[0] for v in global_sums.values()] + [0])
    schema = rare_event_schema(thresholds, strategy_arrow, _observations_arrow(max_obs))

    def row(level: str, unit: str, strategy, players: int, v: list[int]) -> dict:
        obs, comp = v[0], v[1]
        r = {"summary_level": level, "observational_unit": unit, "strategy": strategy, "n_players": players,
             "termination_status": pd.NA, "margin_runner_up": pd.NA, "score_spread": pd.NA, "observations": obs,
             "completed_observations": comp, "safety_limit_observations": v[2],
             "multi_reached_target": v[3] / obs if obs else float("nan")}
        for t, n in zip(thresholds, v[4:]):
            r[f"margin_le_{t}"] = n / comp if comp else float("nan")
        return r

    rows = [row("strategy", STRATEGY_UNIT, sid, players, v) for (sid, players), v in sorted(strategy_sums.items())]
    rows += [row("n_players", GAME_UNIT, pd.NA, players, v) for players, v in sorted(global_sums.items())]
    frame = pd.DataFrame(rows, columns=schema.names)
    frame["strategy"] = frame["strategy"].astype("Int64").array
    for name in ("n_players", "observations", "completed_observations", "safety_limit_observations"):
        frame[name] = frame[name].astype(np.int64)
    return pa.Table.from_pandas(frame, preserve_index=False, schema=schema)
