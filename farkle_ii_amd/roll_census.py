"""The roll census: simulated rolls against the exact dice law, per strategy.

``Engine.census_games`` / ``Engine.tournament_census`` (``fk_census_games`` / ``fk_tournament_run_census``, ``csrc/fk_census.h``) play
games on the device and return four exact integer tables instead of rows or events:

* ``roll_cells [6][61][7]`` — rolls by (dice rolled - 1, raw score / 50, raw dice used).  "Raw" is the roll's maximum immediate score
  and its scoring dice before Smart-5 / Smart-1 discards: ``score_roll_cached(outcome)[:2]`` of the reference
  (src/farkle/analysis/roll_enumeration.py:69);
* ``strategy_dice [S][6][3]`` — for the strategy at turn, by dice rolled - 1: rolls, farkles, rolls in which every die scored;
* ``strategy_turns [S][3]`` — turns, turns that ended on a farkle, the sum of the turns' final ``turn_score`` in points;
* ``turn_hist [S][turn_bins]`` — turns by final ``turn_score`` / 50, clamped to the last bin.

This module holds them (``RollCensus``), states them on the host from ``fk_roll_event`` records alone (``RollCensus.from_events``: what
the device tables are pinned against), restates the reference's exact ordered-roll enumeration (``enumerate_ordered_roll_outcomes``:
its two frames, bit for bit) and builds the frames ``farkle run --roll-census`` writes: the observed distribution beside the exact law,
the per-dice-count fit and the per-strategy turn table.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from itertools import product
from typing import Sequence

import numpy as np

from .backend import CENSUS_ROLL_SHAPE, CENSUS_TABLES, EVENT_DTYPE

SCORE_UNIT = 50
SELECTION_RULE = "production_max_immediate_score_v1"  # roll_enumeration.py:21
DICE_COLS = ("rolls", "farkles", "all_scoring")
TURN_COLS = ("turns", "farkle_turns", "turn_score_sum")
DEFAULT_TURN_BINS = 256
EV_ROLL_AGAIN = 2
TURN_QUANTILES = (("p10_turn_score", 0.1), ("median_turn_score", 0.5), ("p90_turn_score", 0.9))


def raw_score(counts: Sequence[int]) -> tuple[int, int]:
    """(maximum immediate score, scoring dice) of a roll with ``counts[f - 1]`` dice of face f, at most six dice: the rule of
    ``score_counts`` (csrc/fk_device.h; src/farkle/game/scoring.py): the four six-dice patterns, else one n-of-a-kind plus lone ones and
    fives."""
    c = [int(v) for v in counts]
    if c == [1, 1, 1, 1, 1, 1]:
        return 1500, 6  # straight
    if sum(1 for v in c if v == 2) == 3:
        return 1500, 6  # three pairs
    if sum(1 for v in c if v == 3) == 2:
        return 2500, 6  # two triplets
    if 4 in c and 2 in c:
        return 1500, 6  # four of a kind and a pair
    score = used = 0
    for face, v in enumerate(c, start=1):
        if v >= 3:  # at most one such face is left here
            score += (300 if face == 1 else 100 * face) if v == 3 else 1000 * (v - 3)
            used += v
            c[face - 1] = 0
    score += 100 * c[0] + 50 * c[4]
    used += c[0] + c[4]
    return score, used


@lru_cache(maxsize=1)
def _outcome_cells() -> tuple[np.ndarray, np.ndarray]:
    """Per packed dice word of ``fk_roll_event.dice`` (3 bits per face in draw order, the dice count in bits 18-20): raw score / 50 and
    raw dice used, -1 where the word is no roll.  All 6 + ... + 6^6 = 55 986 ordered outcomes."""
    score50 = np.full(1 << 21, -1, dtype=np.int16)
    used = np.full(1 << 21, -1, dtype=np.int16)
    by_counts: dict[tuple, tuple[int, int]] = {}
    for n in range(1, 7):
        for outcome in product(range(1, 7), repeat=n):
            counts = [0] * 6
            word = n << 18
            for i, f in enumerate(outcome):
                counts[f - 1] += 1
                word |= f << (3 * i)
            key = tuple(counts)
            if key not in by_counts:
                by_counts[key] = raw_score(key)
            s, u = by_counts[key]
            score50[word], used[word] = s // SCORE_UNIT, u
    return score50, used


@lru_cache(maxsize=1)
def exact_cells() -> np.ndarray:
    """The exact law as counts: int64 ``[6][61][7]`` ordered outcomes of n dice per (n - 1, raw score / 50, raw used); row n - 1 sums to
    6^n."""
    score50, used = _outcome_cells()
    words = np.flatnonzero(score50 >= 0)
    cells = np.zeros(CENSUS_ROLL_SHAPE, dtype=np.int64)
    np.add.at(cells, ((words >> 18) - 1, score50[words], used[words]), 1)
    cells.setflags(write=False)
    return cells


def _histogram_quantile(values: np.ndarray, counts: np.ndarray, total: int, probability: float) -> float:
    """The linear-interpolation quantile of a population given as ascending ``values`` with integer ``counts``: between the order
    statistics at floor and floor + 1 of ``(total - 1) * probability`` (roll_enumeration.py:36-53; NumPy's default method)."""
    rank = (total - 1) * probability
    lower_rank = int(rank)
    upper_rank = min(lower_rank + 1, total - 1)
    cumulative = np.cumsum(counts)
    lower = int(values[int(np.searchsorted(cumulative, lower_rank, side="right"))])
    upper = int(values[int(np.searchsorted(cumulative, upper_rank, side="right"))])
    return lower + (rank - lower_rank) * (upper - lower)


def enumerate_ordered_roll_outcomes():
    """The reference's ``enumerate_ordered_roll_outcomes()`` (roll_enumeration.py:56-110): the exact distribution frame — one row per
    (dice_count, max_immediate_score, scoring_dice) of the 6^d ordered outcomes of d = 1 .. 6 dice, 127 rows — and the per-dice-count
    summary frame; schema, row order and floats equal to the reference's bit for bit."""
    import pandas as pd

    cells = exact_cells()
    dist: dict[str, list] = {name: [] for name in ("dice_count", "scoring_selection_rule", "max_immediate_score", "scoring_dice", "is_farkle",
                                                    "is_hot_dice", "ordered_outcome_count", "ordered_outcome_probability")}
    summ: dict[str, list] = {name: [] for name in ("dice_count", "scoring_selection_rule", "ordered_outcomes", "farkle_count",
                                                    "farkle_probability", "expected_max_immediate_score", "p10_max_immediate_score",
                                                    "median_max_immediate_score", "p90_max_immediate_score", "hot_dice_probability",
                                                    "expected_scoring_dice")}
    for d in range(1, 7):
        outcomes = 6 ** d
        total_score = total_used = hot = 0
        s50, used = np.nonzero(cells[d - 1])  # ascending (score, used): the reference's sorted cell keys
        for s, u in zip(s50.tolist(), used.tolist()):
            count = int(cells[d - 1, s, u])
            score = s * SCORE_UNIT
            is_hot = score > 0 and u == d
            dist["dice_count"].append(d)
            dist["scoring_selection_rule"].append(SELECTION_RULE)
            dist["max_immediate_score"].append(score)
            dist["scoring_dice"].append(u)
            dist["is_farkle"].append(score == 0)
            dist["is_hot_dice"].append(is_hot)
            dist["ordered_outcome_count"].append(count)
            dist["ordered_outcome_probability"].append(count / outcomes)
            total_score += score * count
            total_used += u * count
            hot += count if is_hot else 0
        by_score = cells[d - 1].sum(axis=1)
        values = np.flatnonzero(by_score) * SCORE_UNIT
        counts = by_score[by_score > 0]
        farkles = int(by_score[0])
        summ["dice_count"].append(d)
        summ["scoring_selection_rule"].append(SELECTION_RULE)
        summ["ordered_outcomes"].append(outcomes)
        summ["farkle_count"].append(farkles)
        summ["farkle_probability"].append(farkles / outcomes)
        summ["expected_max_immediate_score"].append(total_score / outcomes)
        summ["p10_max_immediate_score"].append(_histogram_quantile(values, counts, outcomes, 0.1))
        summ["median_max_immediate_score"].append(_histogram_quantile(values, counts, outcomes, 0.5))
        summ["p90_max_immediate_score"].append(_histogram_quantile(values, counts, outcomes, 0.9))
        summ["hot_dice_probability"].append(hot / outcomes)
        summ["expected_scoring_dice"].append(total_used / outcomes)
    return pd.DataFrame(dist), pd.DataFrame(summ)


@dataclass
class RollCensus:
    """The four tables of a census, int64 (module docstring)."""

    roll_cells: np.ndarray
    strategy_dice: np.ndarray
    strategy_turns: np.ndarray
    turn_hist: np.ndarray

    def __post_init__(self) -> None:
        for name in CENSUS_TABLES:
            setattr(self, name, np.asarray(getattr(self, name), dtype=np.int64))
        S = self.n_strategies
        want = (CENSUS_ROLL_SHAPE, (S, 6, 3), (S, 3), (S, self.turn_bins))
        for name, shape in zip(CENSUS_TABLES, want):
            if getattr(self, name).shape != shape:
                raise ValueError(f"{name} has shape {getattr(self, name).shape}, expected {shape}")

    @property
    def n_strategies(self) -> int:
        return int(self.strategy_turns.shape[0])

    @property
    def turn_bins(self) -> int:
        return int(self.turn_hist.shape[1])

    @classmethod
    def zeros(cls, n_strategies: int, turn_bins: int = DEFAULT_TURN_BINS) -> "RollCensus":
        S = int(n_strategies)
        return cls(np.zeros(CENSUS_ROLL_SHAPE, np.int64), np.zeros((S, 6, 3), np.int64), np.zeros((S, 3), np.int64),
                   np.zeros((S, int(turn_bins)), np.int64))

    @classmethod
    def from_engine(cls, tables: dict) -> "RollCensus":
        """From what ``Engine.census_games`` / ``Engine.tournament_census`` return."""
        return cls(*(tables[name] for name in CENSUS_TABLES))

    def merge(self, other: "RollCensus") -> "RollCensus":
        """The census of both game sets (same table size and ``turn_bins``): every table adds."""
        if other.n_strategies != self.n_strategies or other.turn_bins != self.turn_bins:
            raise ValueError("censuses of different table size or turn_bins do not merge")
        return RollCensus(*(getattr(self, name) + getattr(other, name) for name in CENSUS_TABLES))

    def equals(self, other: "RollCensus") -> bool:
        return all(np.array_equal(getattr(self, name), getattr(other, name)) for name in CENSUS_TABLES)

    def outside_support(self) -> int:
        """Rolls counted in cells the exact law gives no outcome: 0 unless the scorer or the counting is wrong."""
        return int(self.roll_cells[exact_cells() == 0].sum())

    @classmethod
    def from_events(cls, events, event_begin, seat_strategy, S: int, turn_bins: int = DEFAULT_TURN_BINS) -> "RollCensus":
        """The host statement of the census: every table from ``fk_roll_event`` records alone (``Engine.trace_games``: ``events``,
        ``event_begin``) and the games' seats (``seat_strategy [n_games][k]``, table indices).  A roll's raw cell comes from the event's
        faces with the host scorer (``raw_score``); a turn ends at the event without ``FK_EV_ROLL_AGAIN`` and is worth that event's
        ``turn_score``; it ended on a farkle when that event's ``points`` are 0."""
        ev = np.asarray(events, dtype=EVENT_DTYPE)
        begin = np.asarray(event_begin, dtype=np.int64)
        n_games = len(begin) - 1
        ss = np.asarray(seat_strategy, dtype=np.int64).reshape(n_games, -1) if n_games else np.zeros((0, 1), np.int64)
        if not 2 <= int(turn_bins) <= 4096:
            raise ValueError("turn_bins must be in [2, 4096]")
        out = cls.zeros(S, turn_bins)
        if len(ev) == 0:
            return out
        if int(begin[-1]) != len(ev):
            raise ValueError(f"event_begin ends at {int(begin[-1])} for {len(ev)} events")
        game = np.repeat(np.arange(n_games), np.diff(begin))
        strategy = ss[game, ev["seat"].astype(np.int64)]
        if strategy.min() < 0 or strategy.max() >= S:
            raise ValueError("seat_strategy names a strategy outside the table")
        score50_of, used_of = _outcome_cells()
        word = ev["dice"].astype(np.int64)
        n = (word >> 18) & 7
        score50, used = score50_of[word].astype(np.int64), used_of[word].astype(np.int64)
        if (score50 < 0).any():
            raise ValueError("an event's dice word is not a roll of one to six dice")
        np.add.at(out.roll_cells, (n - 1, score50, used), 1)
        np.add.at(out.strategy_dice, (strategy, n - 1, 0), 1)
        farkle = score50 == 0
        np.add.at(out.strategy_dice, (strategy[farkle], n[farkle] - 1, 1), 1)
        hot = used == n
        np.add.at(out.strategy_dice, (strategy[hot], n[hot] - 1, 2), 1)
        last = (ev["flags"] & EV_ROLL_AGAIN) == 0
        who, turn = strategy[last], ev["turn_score"][last].astype(np.int64)
        np.add.at(out.strategy_turns, (who, 0), 1)
        np.add.at(out.strategy_turns, (who[ev["points"][last] == 0], 1), 1)
        np.add.at(out.strategy_turns, (who, 2), turn)
        np.add.at(out.turn_hist, (who, np.minimum(turn // SCORE_UNIT, int(turn_bins) - 1)), 1)
        return out


def observed_roll_distribution(census: RollCensus):
    """One row per (dice_count, max_immediate_score, scoring_dice) of the exact law's support, in its order: the observed count of the
    census, the rolls at that dice count, the observed and the exact probability and the expected count ``rolls x exact probability``.
    Raises when the census counts a roll outside the support."""
    import pandas as pd

    if census.outside_support():
        raise ValueError(f"{census.outside_support()} rolls lie outside the support of the exact law")
    exact = exact_cells()
    rows = []
    for d in range(1, 7):
        rolls = int(census.roll_cells[d - 1].sum())
        outcomes = 6 ** d
        s50, used = np.nonzero(exact[d - 1])
        for s, u in zip(s50.tolist(), used.tolist()):
            count, p = int(census.roll_cells[d - 1, s, u]), int(exact[d - 1, s, u]) / outcomes
            rows.append({"dice_count": d, "max_immediate_score": s * SCORE_UNIT, "scoring_dice": u, "is_farkle": s == 0,
                         "is_hot_dice": s > 0 and u == d, "observed_count": count, "rolls": rolls,
                         "observed_probability": count / rolls if rolls else float("nan"), "ordered_outcome_probability": p,
                         "expected_count": rolls * p})
    return pd.DataFrame(rows)


def roll_fit(census: RollCensus):
    """One row per dice count: the rolls, the cells of the exact law, Pearson's X^2 of the observed cells against it with its degrees
    of freedom (cells - 1) and ``scipy.stats.chi2.sf``, and the observed beside the exact farkle and hot-dice probabilities.

    The number of rolls at a dice count is not fixed in advance: it is random and depends on the outcomes themselves (a farkle ends the
    turn, hot dice bring six dice back, the strategies decide on what they rolled), and the rolls of a game share seat streams.  The
    p-value is therefore a diagnostic — a wrong scorer, dice stream or counter moves it to 0 at once — and not a test at a stated
    level."""
    import pandas as pd
    from scipy.stats import chi2

    if census.outside_support():
        raise ValueError(f"{census.outside_support()} rolls lie outside the support of the exact law")
    exact = exact_cells()
    rows = []
    for d in range(1, 7):
        support = exact[d - 1] > 0
        outcomes = 6 ** d
        observed = census.roll_cells[d - 1][support].astype(np.float64)
        p = exact[d - 1][support] / outcomes
        rolls = int(census.roll_cells[d - 1].sum())
        cells = int(support.sum())
        hot_cells = np.zeros_like(support)
        hot_cells[1:, d] = True
        x2 = float((((observed - rolls * p) ** 2) / (rolls * p)).sum()) if rolls else float("nan")
        rows.append({"dice_count": d, "rolls": rolls, "cells": cells, "chi2": x2, "dof": cells - 1,
                     "p_value": float(chi2.sf(x2, cells - 1)) if rolls else float("nan"),
                     "observed_farkle_probability": int(census.roll_cells[d - 1, 0].sum()) / rolls if rolls else float("nan"),
                     "farkle_probability": int(exact[d - 1, 0].sum()) / outcomes,
                     "observed_hot_dice_probability": int(census.roll_cells[d - 1][hot_cells].sum()) / rolls if rolls else float("nan"),
                     "hot_dice_probability": int(exact[d - 1][hot_cells].sum()) / outcomes})
    return pd.DataFrame(rows)


def _turn_quantile(hist: np.ndarray, q: float) -> float:
    """The smallest turn score s with P(turn_score <= s) >= q, from the histogram of turn_score / 50 (turn scores are multiples of 50,
    so the bins are exact); NaN without a turn and where the answer is the clamp bin."""
    total = int(hist.sum())
    if total == 0:
        return float("nan")
    b = int(np.searchsorted(np.cumsum(hist), math.ceil(q * total), side="left"))
    return float("nan") if b >= len(hist) - 1 else float(b * SCORE_UNIT)


def strategy_turn_table(census: RollCensus, strategy_ids: Sequence[int]):
    """One row per strategy of the table: turns, the rate of turns that ended on a farkle, mean points per turn (exact: the device sums
    the points, the histogram's clamp loses nothing), rolls per turn, the farkle rate by dice rolled and turn-score quantiles from the
    histogram (NaN where the clamp bin is reached)."""
    import pandas as pd

    ids = [int(v) for v in strategy_ids]
    if len(ids) != census.n_strategies:
        raise ValueError(f"{len(ids)} strategy ids for a census of {census.n_strategies} strategies")
    nan = float("nan")
    rows = []
    for i, sid in enumerate(ids):
        turns, farkle_turns, points = (int(v) for v in census.strategy_turns[i])
        dice = census.strategy_dice[i]
        rolls = int(dice[:, 0].sum())
        row = {"strategy": sid, "turns": turns, "farkle_turns": farkle_turns, "farkle_turn_rate": farkle_turns / turns if turns else nan,
               "mean_turn_score": points / turns if turns else nan, "rolls": rolls, "rolls_per_turn": rolls / turns if turns else nan}
        for d in range(1, 7):
            row[f"rolls_{d}_dice"] = int(dice[d - 1, 0])
            row[f"farkle_rate_{d}_dice"] = int(dice[d - 1, 1]) / int(dice[d - 1, 0]) if dice[d - 1, 0] else nan
        for name, q in TURN_QUANTILES:
            row[name] = _turn_quantile(census.turn_hist[i], q)
        rows.append(row)
    return pd.DataFrame(rows)


def observed_table(censuses_by_k: dict):
    """``roll_outcome_distribution_observed.parquet``: ``observed_roll_distribution`` of every player count's census merged
    (``n_players`` 0), then per player count in ascending order."""
    import pandas as pd

    parts = []
    merged = None
    for k in sorted(censuses_by_k):
        merged = censuses_by_k[k] if merged is None else RollCensus(merged.roll_cells + censuses_by_k[k].roll_cells, merged.strategy_dice,
                                                                    merged.strategy_turns, merged.turn_hist)
    for k, census in [(0, merged)] + [(int(k), censuses_by_k[k]) for k in sorted(censuses_by_k)]:
        frame = observed_roll_distribution(census)
        frame.insert(0, "n_players", k)
        parts.append(frame)
    return pd.concat(parts, ignore_index=True)


def fit_table(censuses_by_k: dict):
    """``roll_fit.parquet``: ``roll_fit`` of the merged roll cells (``n_players`` 0), then per player count."""
    import pandas as pd

    cells = sum(c.roll_cells for c in censuses_by_k.values())
    any_census = next(iter(censuses_by_k.values()))
    merged = RollCensus(cells, any_census.strategy_dice, any_census.strategy_turns, any_census.turn_hist)
    parts = []
    for k, census in [(0, merged)] + [(int(k), censuses_by_k[k]) for k in sorted(censuses_by_k)]:
        frame = roll_fit(census)
        frame.insert(0, "n_players", k)
        parts.append(frame)
    return pd.concat(parts, ignore_index=True)


__all__ = ["RollCensus", "raw_score", "exact_cells", "enumerate_ordered_roll_outcomes", "observed_roll_distribution", "roll_fit",
           "strategy_turn_table", "observed_table", "fit_table", "DEFAULT_TURN_BINS", "SELECTION_RULE"]
