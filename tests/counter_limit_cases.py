"""Games that sit at the last value a counter field holds, found on the CPU oracle (test helper, not a conftest).

The game kernels keep the per-seat counters of a row in 16-bit fields with guard bands (csrc/fk_device.h, ``roll_guards50``: more than
64 000 rolls, more than 63 000 returned dice of either kind or more than 65 500 points in a turn is ``FK_ERR_COUNTER_OVERFLOW``); the hot /
cold kernel keeps them in narrower fields whose top bit is a guard bit (``HC_GUARDS`` below, csrc/fk_device.h: the cold record), and a call
that reaches one is replayed on ``fk_play_kernel``; the trace and census kernels refuse a game with more than 65 535 rolls of one seat.

The counters of a fixed game only grow with its round limit, and ``max_rounds`` can be overridden per game, so one game of a call can be
played to R rounds while every other game stops after a handful: ``boundary`` bisects R on the oracle for the largest round limit at which
a field is still within a limit.  The long games are chosen so that the field then holds exactly the limit (64 000 rolls in the play
kernels' calls, 65 535 in the trace and census lists) and passes it in the next round.  The tables are never-banking ones (every turn ends in a farkle: 3.99 rolls per round and seat) in each
flag form of ``kernel_instances.FORMS``, and the one that banks after every roll once it is on the board.

What cannot be reached.  Over all legal flag forms no strategy returns more than 0.61 smart-five dice or 0.31 smart-one dice per roll, so
the two 63 000 dice bands and the 1 310 x 50 turn-score band of the play kernels cannot be reached before the 64 000 rolls band: they stay
checked on the host only (tests/native/roll_guards_host_check.hip).  Of the seven guard bits of the cold record only the farkle bit is
reached first by any game of the search space below (``HOT_COLD_SEARCH``): a game is long only while nobody banks much, and then every
turn is a farkle, which reaches 256 before 3.99 rolls per turn reach 2 048.
"""
from __future__ import annotations

import itertools
from functools import lru_cache

import numpy as np

import kernel_instances as ki

PLAY_ROLLS_LIMIT = 64_000   # RG_N_ROLLS of csrc/fk_device.h: a seat may hold this many rolls, one more is the error
U16_LIMIT = 65_535          # the trace / census kernels' limit, and the oracle's own (its rows are u16)
NEVER_SCORE = 10 ** 6       # a score threshold no turn reaches (a turn above 65 500 points is an error of its own)

# field of a row -> the value whose guard bit the cold record of the hot / cold kernel sets (csrc/fk_device.h:888-897)
HC_GUARDS = {"rolls": 2048, "farkles": 256, "smart_five_uses": 512, "n_smart_five_dice": 1024, "n_smart_one_dice": 1024,
             "smart_one_uses": 512, "hot_dice": 256}


def _po():
    import pyoracle

    return pyoracle


def _blank(S: int) -> np.ndarray:
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    t = np.zeros(S, dtype=STRATEGY_DTYPE)
    t["strategy_id"] = np.arange(S)
    return t


def _checked(table: np.ndarray, form: str) -> np.ndarray:
    ki.check_legal(table)
    assert ki.table_form(table) == form, (form, ki.table_form(table))
    return table


def never_bank_table(form: str, S: int) -> np.ndarray:
    """S strategies that roll until they farkle, of flag form ``form``: the dice threshold -1 asks for another roll with any number of
    dice left, and the score threshold is either not considered, out of reach, or overruled by ``require_both`` (roll on while either
    threshold asks for it)."""
    t = _blank(S)
    i = np.arange(S)
    t["consider_dice"], t["dice_threshold"] = 1, -1
    if form == "none":
        pass  # only the dice threshold is considered
    else:
        t["consider_score"], t["score_threshold"] = 1, NEVER_SCORE
        t["require_both"], t["favor_score"] = i & 1, (i >> 1) & 1
        if form == "all":
            t["auto_hot_dice"], t["smart_five"] = (i >> 2) & 1, (i >> 3) & 1
            t["smart_one"] = t["smart_five"] & ((i >> 4) & 1)
            t["run_up_score"] = (i // 5) & 1
            t["score_threshold"] = np.where(t["require_both"] == 1, 300 * (i % 7), NEVER_SCORE)  # overruled by the dice threshold
    return _checked(t, form)


def bank_at_once_table(S: int) -> np.ndarray:
    """S strategies that bank after every scoring roll once they are on the board (score threshold 0): a roll per turn, about 389 points
    per round — the banked total reaches any target with every counter far inside its field."""
    t = _blank(S)
    t["consider_score"], t["score_threshold"] = 1, 0
    return _checked(t, "none")


# ---- one game of a tournament call played to R rounds --------------------------------------------------------------------------------

def game_override(root: int, shuffle: int, game: int, k: int, rounds: int) -> tuple:
    return (root, shuffle, game, k, rounds)


def game_row(table: np.ndarray, k: int, root: int, shuffle: int, game: int, rounds: int, target: int = 10_000):
    """The oracle's row of game (shuffle, game) with a round limit of ``rounds``, or None where the oracle refuses (a counter beyond u16)."""
    po = _po()
    ov = po.make_overrides([game_override(root, shuffle, game, k, rounds)])
    try:
        ref = po.tournament(np.ascontiguousarray(table).view(po.STRATEGY_DTYPE), k, root, shuffle, shuffle + 1, target_score=target,
                            max_rounds=1, overrides=ov, want_rows=True)
    except po.OracleError:
        return None
    return ref["rows"][game].copy()


def field_max(row, field: str) -> int:
    return int(row["seats"][field].max())


def _bisect(inside, guess: int) -> tuple[int, int]:
    """(R_in, R_out) of a predicate that holds up to some round limit near ``guess`` and never after it."""
    lo, hi = guess, guess
    step = 64
    while not inside(lo):
        assert lo > 0
        hi, lo, step = lo, max(lo - step, 0), step * 4
    while hi == lo or inside(hi):
        assert hi < U16_LIMIT
        lo, hi, step = hi, min(hi + step, U16_LIMIT), step * 4
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if inside(mid) else (lo, mid)
    return lo, hi


def boundary(table: np.ndarray, k: int, root: int, shuffle: int, game: int, field: str, limit: int, target: int = 10_000,
             guess: int | None = None) -> dict:
    """``R_in``: the largest round limit at which the maximum of ``field`` over the seats of game (shuffle, game) is <= ``limit``;
    ``R_out = R_in + 1``; ``row_in`` / ``row_out`` the oracle's rows at both (``row_out`` None where the oracle refuses).  The game must
    not end before ``R_out`` rounds (asserted).  ``guess``: a round limit to start the bracket at."""
    def inside(rounds: int) -> bool:
        row = game_row(table, k, root, shuffle, game, rounds, target)
        return row is not None and field_max(row, field) <= limit

    lo, hi = _bisect(inside, max(min(int(guess or limit // 4), U16_LIMIT - 1), 1))
    row_in, row_out = game_row(table, k, root, shuffle, game, lo, target), game_row(table, k, root, shuffle, game, hi, target)
    assert int(row_in["n_rounds"]) == lo, "the game ends before the field leaves its limit"
    return {"R_in": lo, "R_out": hi, "row_in": row_in, "row_out": row_out}


# ---- the tournament cases of the GPU file -------------------------------------------------------------------------------------------

ROOT = 7
CALL = {"begin": 0, "end": 3, "spb": 2, "max_rounds": 6}   # three shuffles in batches of two, every game but one stops after six rounds
OFFENDER_SHUFFLE = 1                                        # the long game sits in the second shuffle of the first batch
# (form, k, S) -> the game of that shuffle played long: the first one (``search_play_offenders``) whose busiest seat holds EXACTLY 64 000
# rolls after ``R_in`` rounds — the last value the guard lets through — and more after ``R_in + 1``
PLAY_OFFENDERS = {
    ("none", 2, 96): 12, ("none", 3, 96): 0, ("none", 4, 96): 1, ("none", 5, 100): 1, ("none", 6, 96): 1, ("none", 7, 98): 4, ("none", 8, 96): 1,
    ("none", 10, 100): 3, ("none", 11, 99): 1,
    ("rb_fav", 2, 96): 12, ("rb_fav", 3, 96): 0, ("rb_fav", 4, 96): 1, ("rb_fav", 5, 100): 1, ("rb_fav", 6, 96): 1, ("rb_fav", 7, 98): 4,
    ("rb_fav", 8, 96): 1, ("rb_fav", 10, 100): 3, ("rb_fav", 11, 99): 1,
    ("all", 2, 96): 0, ("all", 3, 96): 0, ("all", 4, 96): 5, ("all", 5, 100): 1, ("all", 6, 96): 1, ("all", 7, 98): 4, ("all", 8, 96): 2,
    ("all", 10, 100): 6, ("all", 11, 99): 0,
}


def search_play_offenders(shapes) -> dict:
    """What ``PLAY_OFFENDERS`` holds, for the (form, k, S) of ``shapes`` (half a minute of oracle time; runs in no test)."""
    found = {}
    for form, k, S in shapes:
        table = never_bank_table(form, S)
        found[(form, k, S)] = next(g for g in range(S // k) if field_max(
            boundary(table, k, ROOT, OFFENDER_SHUFFLE, g, "rolls", PLAY_ROLLS_LIMIT, guess=15_000)["row_in"], "rolls") == PLAY_ROLLS_LIMIT)
    return found


@lru_cache(maxsize=None)
def play_case(form: str, k: int, S: int) -> dict:
    """The never-banking table of ``form``, and the round limits around the 64 000-rolls band for the long game of the call ``CALL``."""
    table = never_bank_table(form, S)
    offender = (OFFENDER_SHUFFLE, PLAY_OFFENDERS[(form, k, S)])
    b = boundary(table, k, ROOT, *offender, "rolls", PLAY_ROLLS_LIMIT, guess=15_000)
    return {"table": table, "k": k, "S": S, "offender": offender, "game": (offender[0] - CALL["begin"]) * (S // k) + offender[1], **b}


def call_reference(table: np.ndarray, k: int, rounds: int | None, root: int = ROOT, call: dict | None = None, offender=(OFFENDER_SHUFFLE, 0),
                   target: int = 10_000, n_threads: int = 4):
    """The oracle's result of the call with game ``offender`` played to ``rounds`` (None: no override)."""
    po = _po()
    call = call or CALL
    ov = po.make_overrides([game_override(root, *offender, k, rounds)] if rounds is not None else [])
    return po.tournament(np.ascontiguousarray(table).view(po.STRATEGY_DTYPE), k, root, call["begin"], call["end"], shuffles_per_batch=call["spb"],
                         target_score=target, max_rounds=call["max_rounds"], overrides=ov, want_rows=True, n_threads=n_threads)


# ---- the head-to-head case: one attempt of one block played to R rounds ---------------------------------------------------------------

H2H_NS = 203            # the coordinate namespace of a head-to-head game's seat streams (oracle/farkle_oracle.c: FKO_NS_H2H_PLAYER)
H2H_ATTEMPTS = 3        # every block plays this many attempts (a never-banking pair completes none), all in one launch
H2H_OFFENDER = (1, 0)   # (block, attempt): pass-local game 3; in every form its busier seat holds exactly 64 000 rolls after R_in rounds


def h2h_game_row(seats: np.ndarray, root: int, pair_id: int, order: int, attempt: int, rounds: int, target: int = 10_000):
    po = _po()
    coord = po.coord(H2H_NS, root, 2, pair_id=pair_id, order=order, game_index=attempt)
    try:
        return po.play_game(coord, np.ascontiguousarray(seats).view(po.STRATEGY_DTYPE), [0, 1], target, rounds)[0].copy()
    except po.OracleError:
        return None


@lru_cache(maxsize=None)
def h2h_case(form: str, S: int) -> dict:
    """S / 2 blocks of the never-banking table of ``form`` (block b seats strategies 2b and 2b + 1, pair id 10 + b, order b & 1), and
    the round limits around the 64 000-rolls band for attempt ``H2H_OFFENDER``."""
    table = never_bank_table(form, S)
    seats = table.reshape(-1, 2)
    n = len(seats)
    pair, order = 10 + np.arange(n, dtype=np.uint64), (np.arange(n) & 1).astype(np.uint32)
    b, attempt = H2H_OFFENDER
    args = (seats[b], ROOT, int(pair[b]), int(order[b]), attempt)

    def inside(rounds: int) -> bool:
        row = h2h_game_row(*args, rounds)
        return row is not None and field_max(row, "rolls") <= PLAY_ROLLS_LIMIT

    r_in, r_out = _bisect(inside, 15_000)
    return {"seats": seats, "pair": pair, "order": order, "game": b * H2H_ATTEMPTS + attempt, "R_in": r_in, "R_out": r_out,
            "override": lambda rounds: (ROOT, int(pair[b]), attempt, int(order[b]), rounds),
            "row_in": h2h_game_row(*args, r_in), "row_out": h2h_game_row(*args, r_out)}


# ---- the chunked calls: the offender in the first or in the last chunk ----------------------------------------------------------------

CHUNKED = {"root": 42, "begin": 100, "end": 700, "spb": 50, "max_rounds": 6, "S": 64}  # the range of tests/test_tournament_call_gpu.py


@lru_cache(maxsize=None)
def chunked_case(k: int, where: str) -> dict:
    """600 shuffles of the 64-strategy never-banking table (form ``all``); the offender is game 1 of the first shuffle (``first``) or
    the last game of the last shuffle (``last``)."""
    table = never_bank_table("all", CHUNKED["S"])
    gps = CHUNKED["S"] // k
    shuffle, game = (CHUNKED["begin"], 1) if where == "first" else (CHUNKED["end"] - 1, gps - 1)
    b = boundary(table, k, CHUNKED["root"], shuffle, game, "rolls", PLAY_ROLLS_LIMIT, guess=15_000)
    return {"table": table, "k": k, "offender": (shuffle, game), "game": (shuffle - CHUNKED["begin"]) * gps + game, **b}


# ---- fields at their real maxima ------------------------------------------------------------------------------------------------------

LEAN_TARGET, HC_TARGET, FULL_TARGET = 3_200_000, 135_000, 3_200_050  # the largest targets of lean records and of the hot / cold kernel
MAXIMA_ROUNDS = 9_000


@lru_cache(maxsize=None)
def maxima_reference(k: int, S: int, target: int):
    """One shuffle of the bank-at-once table played to ``target``: (table, the oracle's result with rows)."""
    po = _po()
    table = bank_at_once_table(S)
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, ROOT, 0, 1, target_score=target, max_rounds=MAXIMA_ROUNDS, want_rows=True, n_threads=4)
    return table, ref


def winners_scores(rows) -> np.ndarray:
    assert (rows["status"] == 0).all()
    return rows["seats"]["score"][np.arange(len(rows)), rows["winner_seat"]]


# ---- trace and census: a game list with two games that leave 16 bits ------------------------------------------------------------------

TRACE_TARGET = LEAN_TARGET
TRACE_NS = 103  # the namespace of a tournament game's seat streams


@lru_cache(maxsize=None)
def trace_case() -> dict:
    """Three two-seat games: game 0 between two bank-at-once strategies (it ends at the target after some 8 200 rounds), games 1 and 2
    between never-banking ones.  ``R_in``: the largest round limit at which every seat holds at most 65 535 rolls (a seat of game 1 and a
    seat of game 2 hold exactly that); at ``R_both = R_in + 1`` both games are beyond it."""
    po = _po()
    from farkle_ii_amd.backend import make_coords

    table = np.concatenate([bank_at_once_table(1), never_bank_table("all", 24)[[8, 9, 24 - 1]]])
    table["strategy_id"] = np.arange(len(table))
    ss = np.array([[0, 0], [3, 1], [1, 2]], dtype=np.int32)
    # games 1 and 2 share their coordinates (found by trying shuffle indices): after R_in rounds a seat of each holds exactly 65 535 rolls
    coords = make_coords(TRACE_NS, ROOT, 2, shuffle_index=np.array([4, 4, 4], dtype=np.uint64), game_index=np.array([0, 1, 1], dtype=np.uint64))

    def rows(games, rounds):
        try:
            return po.play_games(coords[games].view(po.COORD_DTYPE), table.view(po.STRATEGY_DTYPE), ss[games], 2, TRACE_TARGET, rounds)
        except po.OracleError:
            return None

    edge = {g: _bisect(lambda r, g=g: rows([g], r) is not None, 15_000)[0] for g in (1, 2)}
    r_in = min(edge.values())
    return {"coords": coords, "table": table, "ss": ss, "R_in": r_in, "first": min(edge, key=edge.get), "R_both": max(edge.values()) + 1,
            "edge": edge, "rows": rows}


# the long game is game 21 of the call, in the second chunk; its busiest seat holds exactly 65 535 rolls after R_in rounds
CENSUS_CALL = {"k": 2, "S": 8, "begin": 0, "end": 8, "max_rounds": 6, "chunk_games": 16, "offender": (5, 1)}


@lru_cache(maxsize=None)
def census_case() -> dict:
    cc = CENSUS_CALL
    table = never_bank_table("all", cc["S"])
    b = boundary(table, cc["k"], ROOT, *cc["offender"], "rolls", U16_LIMIT, guess=16_000)
    return {"table": table, "game": (cc["offender"][0] - cc["begin"]) * (cc["S"] // cc["k"]) + cc["offender"][1], **b}


# ---- the hot / cold guard bits: which field reaches its bit first ---------------------------------------------------------------------
#
# The search space (``search_hot_cold``; its result is the data below, the search itself runs in no test): every legal flag form
# (smart_one only with smart_five, require_both only with both thresholds considered: 120 forms) x score thresholds
# {0, 50 .. 400 in steps of 50, 500, 750, 1 000, 3 000, 10^6} x dice thresholds -1 .. 5, one strategy seated four times (k = 4, so that nobody else ends the game), root 7,
# game (0, 0), target 135 000 (the largest the hot / cold kernel plays), round limits up to 1 100 (a never-banking seat holds 256 farkles
# after 256 rounds; no game of the space lasts longer than that with every field below its bit).  For each of the 11 760 strategies the
# game is cut at the last round limit with every field of every seat below its guard bit; ``closest`` is the largest value / bit a field
# shows there, ``first`` a strategy whose next round takes that field (and no other) to its bit.

HOT_COLD_SEARCH = {
    "space": {"k": 4, "root": ROOT, "shuffle": 0, "game": 0, "target": 135_000, "score_thresholds": (0, 50, 100, 150, 200, 250, 300, 350, 400, 500, 750, 1000, 3000, NEVER_SCORE),
              "dice_thresholds": tuple(range(-1, 6)), "round_limit": 1100},
    # the result of search_hot_cold()
    "fields": {
        "rolls": {"reachable": False, "closest": 0.7368, "R": 369, "strategy": (350, 1, 1, 1, 1, 1, 1, 1, 1, 0)},
        "farkles": {"reachable": True, "closest": 1.0, "R": 255, "strategy": (0, -1, 0, 0, 0, 1, 0, 0, 0, 0)},
        "smart_five_uses": {"reachable": False, "closest": 0.8789, "R": 369, "strategy": (350, 1, 1, 1, 1, 1, 1, 1, 1, 0)},
        "n_smart_five_dice": {"reachable": False, "closest": 0.5273, "R": 369, "strategy": (350, 1, 1, 1, 1, 1, 1, 1, 1, 0)},
        "n_smart_one_dice": {"reachable": False, "closest": 0.2402, "R": 372, "strategy": (3000, 1, 1, 1, 1, 1, 0, 1, 1, 0)},
        "smart_one_uses": {"reachable": False, "closest": 0.459, "R": 372, "strategy": (3000, 1, 1, 1, 1, 1, 0, 1, 0, 0)},
        "hot_dice": {"reachable": False, "closest": 0.5703, "R": 255, "strategy": (1000000, 5, 1, 0, 1, 1, 1, 1, 1, 0)},
    },
}


def legal_flag_forms():
    """The 120 legal flag vectors, as dicts."""
    for sf, so, cs, cd, rb, hot, run_up, fav in itertools.product((0, 1), repeat=8):
        if (so and not sf) or (rb and not (cs and cd)):
            continue
        yield {"smart_five": sf, "smart_one": so, "consider_score": cs, "consider_dice": cd, "require_both": rb, "auto_hot_dice": hot,
               "run_up_score": run_up, "favor_score": fav}


STRATEGY_FIELDS = ("score_threshold", "dice_threshold", *ki.FLAG_NAMES)  # the order of a strategy tuple in the search's result


def uniform_table(strategy, S: int) -> np.ndarray:
    """S copies of one strategy (a dict, or a tuple in the order of ``STRATEGY_FIELDS``)."""
    t = _blank(S)
    for name, value in (strategy.items() if isinstance(strategy, dict) else zip(STRATEGY_FIELDS, strategy)):
        t[name] = value
    return _checked(t, "none")


def hot_cold_cut(strategy: dict, space: dict | None = None) -> dict:
    """The game of the search space for ``strategy``, cut at the last round limit ``R`` with every field below its guard bit: ``ratios``
    (field -> largest value / bit at R) and ``crossing`` (the fields at or above their bit at R + 1; empty when the game ends first)."""
    sp = space or HOT_COLD_SEARCH["space"]
    table = uniform_table(strategy, sp["k"])
    args = (table, sp["k"], sp["root"], sp["shuffle"], sp["game"])

    def over(row) -> list[str]:
        return [f for f, bit in HC_GUARDS.items() if field_max(row, f) >= bit]

    full = game_row(*args, sp["round_limit"], sp["target"])
    assert full is not None
    lo, hi = 0, int(full["n_rounds"])
    if not over(full):
        cut, crossing = full, []
        lo = hi
    else:
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if over(game_row(*args, mid, sp["target"])):
                hi = mid
            else:
                lo = mid
        cut, crossing = game_row(*args, lo, sp["target"]), over(game_row(*args, hi, sp["target"]))
    return {"R": lo, "ratios": {f: field_max(cut, f) / bit for f, bit in HC_GUARDS.items()}, "crossing": crossing}


def search_hot_cold() -> dict:
    """Runs the search (about twenty seconds of oracle time) and returns what ``HOT_COLD_SEARCH["fields"]`` holds."""
    sp = HOT_COLD_SEARCH["space"]
    best = {f: {"reachable": False, "closest": 0.0, "strategy": None, "R": 0} for f in HC_GUARDS}
    for flags in legal_flag_forms():
        for st in sp["score_thresholds"]:
            for dt in sp["dice_thresholds"]:
                strategy = (st, dt, *(flags[name] for name in ki.FLAG_NAMES))
                cut = hot_cold_cut(strategy, sp)
                for f in HC_GUARDS:
                    b = best[f]
                    alone = cut["crossing"] == [f]
                    if alone and not b["reachable"]:
                        best[f] = {"reachable": True, "closest": 1.0, "strategy": strategy, "R": cut["R"]}
                    elif not b["reachable"] and cut["ratios"][f] > b["closest"]:
                        best[f] = {"reachable": False, "closest": round(cut["ratios"][f], 4), "strategy": strategy, "R": cut["R"]}
    return best


def hot_cold_cases() -> dict:
    """field -> {"strategy", "R"} for the fields a game of the search space takes to their guard bit first (R: the last round limit
    below the bit; R + 1 reaches it)."""
    return {f: v for f, v in HOT_COLD_SEARCH["fields"].items() if v["reachable"]}


if __name__ == "__main__":
    import pprint

    pprint.pprint(search_hot_cold(), width=150, sort_dicts=False)
