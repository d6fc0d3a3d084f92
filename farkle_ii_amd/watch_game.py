"""``farkle watch``: one game, every roll, scoring call and decision logged (``src/farkle/simulation/watch_game.py``).

The reference wraps its engine — a ``TracePlayer`` logs ``_roll`` (:141-153), ``patch_scoring`` logs ``default_score`` (:97-138),
``_trace_decide`` logs ``strategy.decide`` (:69-94) — and plays one two-player game (:157-221).  Here the game is played on the
device by ``fk_trace_games`` and the same messages are formatted from its roll events (``render``); ``watch_game`` logs them, in
the reference's order, with ``extra={"stage": "watch"}``.
"""
from __future__ import annotations

import logging
from dataclasses import asdict
from typing import Sequence

import numpy as np

from . import trace
from .backend import make_coords
from .random import RandomPurpose, coordinate_rng
from .strategies import ThresholdStrategy, pack_strategies, random_threshold_strategy

LOGGER = logging.getLogger(__name__)
FINAL_RESULT = "\n===== final result ====="


def strategy_yaml(strategy: ThresholdStrategy) -> str:
    """The dataclass fields in declaration order, YAML-like (watch_game.py:35-66)."""
    if not isinstance(strategy, ThresholdStrategy):
        raise TypeError("strategy_yaml expects a ThresholdStrategy")
    return "\n".join(f"{k:<15}: {str(v).lower() if isinstance(v, bool) else v}" for k, v in asdict(strategy).items())


def render_rolls(events) -> list[str]:
    """Per roll: ``P# rolls [..]``, ``score([..]) -> pts=.. used=.. reroll=..`` and, where ``decide`` was consulted, its line.
    (``decide``'s answer is the event's roll-again bit: the override of engine.py:202 only fires where it already said ROLL.)"""
    ev = np.asarray(events, dtype=trace.EVENT_DTYPE)
    out: list[str] = []
    for roll, seat, pts, used, left, turn, flags in zip(trace.faces(ev), ev["seat"].tolist(), ev["points"].tolist(), trace.used(ev).tolist(),
                                                        trace.dice_left(ev).tolist(), ev["turn_score"].tolist(), ev["flags"].tolist()):
        out.append(f"P{seat + 1} rolls {roll}")
        out.append(f"score({roll}) -> pts={pts:<4} used={used} reroll={len(roll) - used}")
        if flags & trace.EV_DECIDE:
            out.append(f"P{seat + 1} decide(): turn={turn} dice_left={left} -> {'ROLL' if flags & trace.EV_ROLL_AGAIN else 'BANK'}")
    return out


def render(events, strategies: Sequence[ThresholdStrategy] | None = None, row=None) -> list[str]:
    """The reference's messages for one traced game: the strategy headers (with ``strategies``), the roll lines, and (with the
    game's ``row``) the result.  The reference cannot format the last record of a safety-limit game (``%d`` of ``None``: its logging
    reports the error and the record is lost); this logs ``Winner: None  score=None  rounds=<n_rounds>`` for it."""
    out = [f"P{i + 1} strategy\n{strategy_yaml(s)}\n" for i, s in enumerate(strategies or ())]
    out += render_rolls(events)
    if row is not None:
        out.append(FINAL_RESULT)
        winner = int(row["winner_seat"])
        if winner < 0:
            out.append(f"Winner: None  score=None  rounds={int(row['n_rounds'])}")
        else:
            out.append(f"Winner: P{winner + 1}  score={int(row['seats'][winner]['score'])}  rounds={int(row['n_rounds'])}")
    return out


def watch_strategies(seed: int) -> list[ThresholdStrategy]:
    return [random_threshold_strategy(coordinate_rng(RandomPurpose.STRATEGY, root_seed=seed, k=2, seat_index=i)) for i in range(2)]


def _log(messages: Sequence[str]) -> None:
    for m in messages:
        LOGGER.info("%s", m, extra={"stage": "watch"})


def watch_game(seed: int | None = None, engine=None) -> None:
    """Play the reference's ``watch_game(seed)`` game — two ``random_threshold_strategy`` of the STRATEGY streams, seat streams of
    namespace PLAYER with ``root_seed=seed, k=2``, target 10 000 — and log its messages.  A safety-limit game ends with
    ``Winner: None  score=None  rounds=200`` (see ``render``)."""
    if seed is None:
        raise ValueError("watch_game requires an explicit seed")
    if engine is None:
        from .engine import get_engine

        engine = get_engine()
    strategies = watch_strategies(seed)
    coords = make_coords(int(RandomPurpose.PLAYER), seed, 2)
    rows, begin, events = engine.trace_games(coords, pack_strategies(strategies), [0, 1], 2, target_score=10_000, max_rounds=200)
    _log(render(events[begin[0]:begin[1]], strategies, rows[0]))


def watch_tournament_game(strategies: Sequence[ThresholdStrategy], root_seed: int, k: int, shuffle_index: int, game_index: int, engine=None,
                          target_score: int = 10_000, max_rounds: int = 200) -> None:
    """Replay game ``game_index`` of shuffle ``shuffle_index`` of a tournament over ``strategies`` and log it like ``watch_game``."""
    if engine is None:
        from .engine import get_engine

        engine = get_engine()
    row, events, seats = trace.trace_tournament_game(engine, pack_strategies(strategies), root_seed, k, shuffle_index, game_index,
                                                     target_score=target_score, max_rounds=max_rounds)
    _log(render(events, [strategies[i] for i in seats.tolist()], row))


__all__ = ["watch_game", "watch_tournament_game", "render", "render_rolls", "strategy_yaml", "watch_strategies"]
