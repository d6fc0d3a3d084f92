"""TEST INFRASTRUCTURE ONLY — the roll events of a game from the CPU oracle's primitives.

The oracle plays whole games (``pyoracle.play_game``) and says nothing about their rolls.  This restates its turn and game loop
(``play_players`` / ``take_turn`` of oracle/farkle_oracle.c, i.e. FarklePlayer.take_turn and FarkleGame.play / _run_final_round of the
reference, src/farkle/game/engine.py:208-273, 436-550) in Python on the oracle's own ``dice_stream``, ``default_score`` and
``should_continue``, and emits one ``fk_roll_event`` per roll plus the game's row.  Every user pins it first by
``row == pyoracle.play_game(...)``: a restatement that gets a roll wrong gets the row wrong.
"""
from __future__ import annotations

import numpy as np
import pyoracle as po

from farkle_ii_amd.backend import EVENT_DTYPE

ROLL_LIMIT = 1000
EV_DECIDE, EV_ROLL_AGAIN, EV_FINAL_ROUND, EV_AUTO_HOT = 1, 2, 4, 8


class _Seat:
    def __init__(self, coord, seat: int, strategy: np.ndarray):
        self.coord = coord.copy()
        self.coord["seat_index"] = seat
        self.strategy = strategy  # one-element view of the table
        self.sizes: list[int] = []
        self.score = 0
        self.has_scored = False
        self.n = dict.fromkeys(("farkles", "rolls", "n_turns", "highest_turn", "smart_five_uses", "n_smart_five_dice", "smart_one_uses",
                                "n_smart_one_dice", "hot_dice"), 0)

    def roll(self, n: int) -> list[int]:
        """The next n dice of the seat's stream (the oracle replays the stream from its coordinate: the tail is the new roll)."""
        self.sizes.append(n)
        return po.dice_stream(self.coord, self.sizes)[-n:].tolist()


def trace_game(coord, table, seat_strategy, target_score: int = 10_000, max_rounds: int = 200):
    """(events, row) of one game; ``coord`` is a one-element COORD_DTYPE array with seat_index 0."""
    table = np.ascontiguousarray(table, dtype=po.STRATEGY_DTYPE)
    ss = [int(v) for v in seat_strategy]
    k = len(ss)
    seats = [_Seat(coord, i, table[ss[i]:ss[i] + 1]) for i in range(k)]
    events: list[tuple] = []
    rounds = 0

    def take_turn(i: int, final_round: bool, score_to_beat: int) -> None:
        p = seats[i]
        s = p.strategy[0]
        p.n["n_turns"] += 1
        dice, turn_score, rolls_this_turn = 6, 0, 0
        while dice > 0:
            if rolls_this_turn >= ROLL_LIMIT:
                raise po.OracleError("oracle error -1: turn exceeded 1000 rolls")
            n = dice
            faces = p.roll(n)
            p.n["rolls"] += 1
            rolls_this_turn += 1
            pts, used, reroll, d5, d1 = po.default_score(faces, turn_score, p.strategy)
            flags = EV_FINAL_ROUND if final_round else 0
            if pts == 0:
                p.n["farkles"] += 1
                turn_score, dice = 0, 0
            else:
                if d5:
                    p.n["smart_five_uses"] += 1
                    p.n["n_smart_five_dice"] += d5
                if d1:
                    p.n["smart_one_uses"] += 1
                    p.n["n_smart_one_dice"] += d1
                dice = 6 if (used == n and reroll == 0) else reroll
                turn_score += pts
                if s["auto_hot_dice"] and dice == 6:
                    p.n["hot_dice"] += 1
                    flags |= EV_AUTO_HOT | EV_ROLL_AGAIN
                else:
                    if not (final_round and p.score + turn_score > score_to_beat and not s["run_up_score"]):
                        flags |= EV_DECIDE
                    if po.should_continue(p.strategy, turn_score, dice, p.has_scored, final_round, score_to_beat, p.score):
                        flags |= EV_ROLL_AGAIN
            packed = sum(f << (3 * j) for j, f in enumerate(faces)) | (n << 18)
            events.append((packed, turn_score, pts, rounds, i, used | (dice << 4), d5 | (d1 << 4), flags))
            if not flags & EV_ROLL_AGAIN:
                break
        if not p.has_scored and turn_score >= 500:
            p.has_scored = True
        if p.has_scored:
            p.score += turn_score
            p.n["highest_turn"] = max(p.n["highest_turn"], turn_score)

    final_round, score_to_beat = False, target_score
    while rounds < max_rounds and not final_round:
        rounds += 1
        for i in range(k):
            take_turn(i, False, score_to_beat)
            if seats[i].score >= target_score:
                final_round, score_to_beat = True, seats[i].score
                for j in range(k):
                    if j != i:
                        take_turn(j, True, score_to_beat)
                        score_to_beat = max(score_to_beat, seats[j].score)
                break
    row = np.zeros(1, dtype=po.row_dtype(k))
    row["n_rounds"] = rounds
    row["status"] = 0 if final_round else 1
    row["winner_seat"] = -1
    for i, p in enumerate(seats):
        rec = row["seats"][0][i]
        rec["score"], rec["strategy"] = p.score, ss[i]
        for name, v in p.n.items():
            rec[name] = v
        rec["hit_max_rounds"] = 0 if final_round else 1
        if final_round:
            rec["rank"] = 1 + sum(1 for j, q in enumerate(seats) if q.score > p.score or (q.score == p.score and j < i))
            if rec["rank"] == 1:
                row["winner_seat"] = i
    return np.array(events, dtype=EVENT_DTYPE), row


def trace_games(coords, table, seat_strategy, k: int, target_score: int = 10_000, max_rounds: int = 200):
    """The stand-in for ``Engine.trace_games``: (rows, event_begin, events)."""
    coords = np.ascontiguousarray(coords, dtype=po.COORD_DTYPE)
    ss = np.ascontiguousarray(seat_strategy, dtype=np.int32).reshape(len(coords), k)
    rows = np.zeros(len(coords), dtype=po.row_dtype(k))
    begin = np.zeros(len(coords) + 1, dtype=np.int64)
    parts = []
    for g in range(len(coords)):
        ev, row = trace_game(coords[g:g + 1], table, ss[g], target_score, max_rounds)
        rows[g] = row[0]
        begin[g + 1] = begin[g] + len(ev)
        parts.append(ev)
    return rows, begin, np.concatenate(parts) if parts else np.zeros(0, dtype=EVENT_DTYPE)


def pinned(coords, table, seat_strategy, k: int, target_score: int = 10_000, max_rounds: int = 200):
    """``trace_games`` after asserting that its rows are the oracle's own rows for the same games."""
    rows, begin, events = trace_games(coords, table, seat_strategy, k, target_score, max_rounds)
    expect = po.play_games(np.ascontiguousarray(coords, dtype=po.COORD_DTYPE), np.ascontiguousarray(table, dtype=po.STRATEGY_DTYPE),
                           seat_strategy, k, target_score, max_rounds)
    assert rows.tobytes() == expect.tobytes(), "the Python restatement of the oracle's game loop disagrees with the oracle"
    return rows, begin, events
