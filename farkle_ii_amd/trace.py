"""Roll-level game traces: decoders of ``fk_roll_event``, the row of a game rebuilt from its events, tournament replay.

``Engine.trace_games`` (``fk_trace_games``, ``csrc/fk_trace.h``) returns, per game of an explicit list, the ordered roll events of
``FarklePlayer.take_turn`` (``src/farkle/game/engine.py:208-273``) inside ``FarkleGame.play`` / ``_run_final_round`` (:436-550).
This module reads them:

* the field decoders (``faces``, ``n_dice``, ``used``, ``dice_left``, ``d5``, ``d1``, ``decided``, ``rolls_again``, ``final_round``,
  ``auto_hot``);
* ``rows_from_events`` rebuilds every field of a game row from its events alone — what a player banks follows from ``has_scored``
  and the 500-point entry rule (engine.py:265-273), ranks from ``(-score, seat)`` (:477-483) — and ``check`` compares such rows
  with the rows a call returned, naming the first game, seat and field that differ;
* ``trace_tournament_game`` replays any game of a tournament from the coordinates its row carries (root seed, k, shuffle, game).
"""
from __future__ import annotations

import numpy as np

from .backend import EVENT_DTYPE, make_coords, row_dtype
from .random import RandomPurpose, coordinate_rng

EV_DECIDE, EV_ROLL_AGAIN, EV_FINAL_ROUND, EV_AUTO_HOT = 1, 2, 4, 8
ENTRY_SCORE = 500  # engine.py:267
SEAT_COUNTERS = ("farkles", "rolls", "n_turns", "highest_turn", "smart_five_uses", "n_smart_five_dice", "smart_one_uses",
                 "n_smart_one_dice", "hot_dice")


def _events(events) -> np.ndarray:
    return np.asarray(events, dtype=EVENT_DTYPE)


def n_dice(events) -> np.ndarray:
    return (_events(events)["dice"] >> 18) & 7


def faces(events) -> list[list[int]]:
    """The dice of every event in draw order, as the reference's ``_roll`` returns them."""
    ev = _events(events)
    return [[int((d >> (3 * i)) & 7) for i in range(int((d >> 18) & 7))] for d in ev["dice"].tolist()]


def used(events) -> np.ndarray:
    return _events(events)["used_left"] & 15


def dice_left(events) -> np.ndarray:
    return _events(events)["used_left"] >> 4


def d5(events) -> np.ndarray:
    return _events(events)["discards"] & 15


def d1(events) -> np.ndarray:
    return _events(events)["discards"] >> 4


def decided(events) -> np.ndarray:
    return (_events(events)["flags"] & EV_DECIDE) != 0


def rolls_again(events) -> np.ndarray:
    return (_events(events)["flags"] & EV_ROLL_AGAIN) != 0


def final_round(events) -> np.ndarray:
    return (_events(events)["flags"] & EV_FINAL_ROUND) != 0


def auto_hot(events) -> np.ndarray:
    return (_events(events)["flags"] & EV_AUTO_HOT) != 0


def rows_from_events(events, event_begin, seat_strategy, k: int, target_score: int = 10_000, max_rounds: int = 200) -> np.ndarray:
    """The rows of the traced games from their events alone (``seat_strategy`` only fills the rows' ``strategy`` field; the strategy
    table is not used).  A turn starts at a game's first event and after an event that does not roll again; a turn's points are the
    ``turn_score`` of its last event; a game without an event in the final round ran into ``max_rounds`` (every completed game's last
    turn is a final-round turn, or — one seat — the turn that reached the target)."""
    ev = _events(events)
    begin = np.asarray(event_begin, dtype=np.int64)
    n = len(begin) - 1
    ss = np.asarray(seat_strategy, dtype=np.int32).reshape(n, k)
    rows = np.zeros(n, dtype=row_dtype(k))
    rows["seats"]["strategy"] = ss
    for g in range(n):
        e = ev[begin[g]:begin[g + 1]]
        seats = rows[g]["seats"]
        score = [0] * k
        has_scored = [False] * k
        count = {name: [0] * k for name in SEAT_COUNTERS}
        rounds = 0
        new_turn = True
        for seat, turn, points, rnd, disc, flags in zip(e["seat"].tolist(), e["turn_score"].tolist(), e["points"].tolist(),
                                                        e["round"].tolist(), e["discards"].tolist(), e["flags"].tolist()):
            if new_turn:
                count["n_turns"][seat] += 1
            count["rolls"][seat] += 1
            rounds = max(rounds, rnd)
            if points == 0:
                count["farkles"][seat] += 1
            if disc & 15:
                count["smart_five_uses"][seat] += 1
                count["n_smart_five_dice"][seat] += disc & 15
            if disc >> 4:
                count["smart_one_uses"][seat] += 1
                count["n_smart_one_dice"][seat] += disc >> 4
            if flags & EV_AUTO_HOT:
                count["hot_dice"][seat] += 1
            new_turn = not flags & EV_ROLL_AGAIN
            if new_turn:  # the turn is over: engine.py:265-273
                if not has_scored[seat] and turn >= ENTRY_SCORE:
                    has_scored[seat] = True
                if has_scored[seat]:
                    score[seat] += turn
                    count["highest_turn"][seat] = max(count["highest_turn"][seat], turn)
        if len(e) and not new_turn:
            raise ValueError(f"game {g}: the last event rolls again")
        completed = any(s >= target_score for s in score)  # somebody triggered the final round (engine.py:462-468)
        if not completed and (len(e) == 0) != (max_rounds == 0):
            raise ValueError(f"game {g}: {len(e)} events at max_rounds = {max_rounds}")
        for i in range(k):
            seats[i]["score"] = score[i]
            for name in SEAT_COUNTERS:
                seats[i][name] = count[name][i]
        rows[g]["n_rounds"] = rounds
        if completed:
            order = sorted(range(k), key=lambda i: (-score[i], i))
            for rank, i in enumerate(order, start=1):
                seats[i]["rank"] = rank
            rows[g]["status"] = 0
            rows[g]["winner_seat"] = order[0]
        else:
            rows[g]["status"] = 1
            rows[g]["winner_seat"] = -1
            seats["hit_max_rounds"] = 1
            if rounds != max_rounds:
                raise ValueError(f"game {g}: a safety-limit game of {rounds} rounds at max_rounds = {max_rounds}")
    return rows


def check(events, event_begin, rows, seat_strategy, k: int, target_score: int = 10_000, max_rounds: int = 200) -> None:
    """Raise ``ValueError`` naming the first game, seat and field at which ``rows`` differ from the rows the events give."""
    rebuilt = rows_from_events(events, event_begin, seat_strategy, k, target_score, max_rounds)
    rows = np.asarray(rows, dtype=row_dtype(k))
    if len(rows) != len(rebuilt):
        raise ValueError(f"{len(rows)} rows for {len(rebuilt)} traced games")
    for g in np.flatnonzero(rows != rebuilt).tolist():
        for name in ("n_rounds", "status", "winner_seat"):
            if rows[g][name] != rebuilt[g][name]:
                raise ValueError(f"game {g}: {name} is {rows[g][name]} in the row, {rebuilt[g][name]} from the events")
        for seat in range(k):
            for name in rows.dtype["seats"].base.names:
                a, b = rows[g]["seats"][seat][name], rebuilt[g]["seats"][seat][name]
                if a != b:
                    raise ValueError(f"game {g} seat {seat}: {name} is {a} in the row, {b} from the events")


def tournament_seats(root_seed: int, k: int, shuffle_index: int, game_index: int, n_strategies: int) -> np.ndarray:
    """Table indices of the seats of one tournament game: ``perm[g * k:(g + 1) * k]`` of the shuffle's permutation
    (src/farkle/simulation/run_tournament.py:301-351)."""
    if n_strategies % k or not 0 <= game_index < n_strategies // k:
        raise ValueError(f"game {game_index} of {n_strategies} strategies at {k} players does not exist")
    perm = coordinate_rng(RandomPurpose.SHUFFLE_PERMUTATION, root_seed=root_seed, k=k, shuffle_index=shuffle_index).permutation(n_strategies)
    return np.asarray(perm[game_index * k:(game_index + 1) * k], dtype=np.int32)


def trace_tournament_game(engine, table, root_seed: int, k: int, shuffle_index: int, game_index: int, target_score: int = 10_000,
                          max_rounds: int = 200):
    """Replay one game of a tournament by the coordinates its row carries: ``(row, events, seats)`` with ``seats`` the table
    indices in seat order.  The seat streams are those of namespace 103 (``TOURNAMENT_PLAYER``) the tournament kernels use."""
    seats = tournament_seats(root_seed, k, shuffle_index, game_index, len(table))
    coords = make_coords(int(RandomPurpose.TOURNAMENT_PLAYER), root_seed, k, shuffle_index=shuffle_index, game_index=game_index)
    rows, begin, events = engine.trace_games(coords, table, seats, k, target_score=target_score, max_rounds=max_rounds)
    return rows[0], events[begin[0]:begin[1]], seats


__all__ = ["EV_DECIDE", "EV_ROLL_AGAIN", "EV_FINAL_ROUND", "EV_AUTO_HOT", "faces", "n_dice", "used", "dice_left", "d5", "d1", "decided",
           "rolls_again", "final_round", "auto_hot", "rows_from_events", "check", "tournament_seats", "trace_tournament_game"]
