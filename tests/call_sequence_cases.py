"""Call sequences on one context: what a call leaves behind for the next one (DESIGN "What outlives a call").

A context keeps two chunk sets, the hint of ``fk_tournament_hint_next``, the table epoch, the row-buffer parity and the rows events,
the shared record buffers, the resident tally and the round-robin accumulator between calls.  The sequences below are DATA: lists of

    ("hint", lo, hi, need_state)     Engine.hint_next
    ("option", name, value)          Engine.set_option
    ("call", kind, params)           one entry of ``KINDS`` (a tournament entry or a neighbour), ``params`` from ``P(...)``

and ``run(engine, steps)`` executes them on any engine: the HIP engine, the combined CPU engine below (every existing CPU stub in
one class), or a deliberately wrong wrapper of it (``StaleEngine``, ``ResidueEngine``: the detector checks).  Every call step is
compared, key by key, with the same call made ALONE on a fresh combined CPU engine (``expected``, cached per (kind, params)).

No GPU is needed to import this module or to run the sequences on the CPU engine."""
from __future__ import annotations

import itertools
import random
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import oracle_engine_stub  # noqa: F401  (first: it puts the repository and the oracle on the path)
import census_engine_stub
import matchup_engine_stub
import perm_stage_cases
import rare_events_engine_stub
import round_robin_engine_stub
import seat_analysis_engine_stub
import trace_engine_stub
from farkle_ii_amd.backend import CENSUS_TABLES, make_coords, make_overrides

LAGS = (1, 2, 7)
GAME_STAT_NAMES = ("strategy_counts", "strategy_rounds", "strategy_runner", "strategy_spread", "game_counts", "game_rounds", "game_runner")
BIG = 48 << 30   # the default chunk_bytes
SMALL = 1 << 20  # the smallest workspace: several chunks per call on the 1 024-strategy table


# ------------------------------------------------------------------------------------------------------------------------ tables
@lru_cache(maxsize=None)
def tables() -> dict:
    """``g64``: the 64-strategy benchmark grid; ``g64b``: another table of 64 (its packed form differs: another epoch);
    ``g1024``: the first 1 024 strategies of the default grid (the multi-chunk cases)."""
    from tools.time_config import table_for

    g64 = table_for(64)
    g64b = g64.copy()
    g64b["score_threshold"][::2] += 100
    out = {"g64": g64, "g64b": g64b, "g1024": table_for(1024)}
    for t in out.values():
        t.setflags(write=False)
    return out


def ids_for(S: int) -> np.ndarray:
    """Unique strategy IDs whose order is not the table's."""
    prime = {64: 257, 1024: 1031}[S]
    return ((np.arange(S, dtype=np.int64) * 37 + 11) % prime).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------- parameters
DEFAULT_OV = ((1, 1, 1), (3, 0, 2))  # (shuffle - lo, game of the shuffle, max_rounds): games that end at their own safety limit


def P(table: str = "g64", k: int = 2, root: int = 42, lo: int = 8, hi: int = 32, target: int = 3000, rounds: int = 9, ov: tuple = DEFAULT_OV,
      copy: bool = False) -> tuple:
    """The parameters of one call, hashable.  ``ov``: overrides relative to ``lo``; ``copy``: the table is passed as a fresh copy."""
    return (("copy", copy), ("hi", hi), ("k", k), ("lo", lo), ("ov", tuple(ov)), ("root", root), ("rounds", rounds), ("table", table),
            ("target", target))


def _lead(p: dict) -> tuple:
    """(table, k, root, lo, hi) and the keyword arguments every tournament entry takes."""
    table = tables()[p["table"]]
    if p["copy"]:
        table = table.copy()
    ov = make_overrides([(p["root"], p["lo"] + a, b, p["k"], r) for a, b, r in p["ov"]])
    return (table, p["k"], p["root"], p["lo"], p["hi"]), dict(target_score=p["target"], max_rounds=p["rounds"], overrides=ov)


# --------------------------------------------------------------------------------------------------------------------------- kinds
@dataclass(frozen=True)
class Kind:
    call: object          # (engine, params dict) -> the entry's result (a dict, possibly nested)
    keys: tuple           # the dotted keys compared: those the entry's own GPU test compares
    tournament: bool      # a tournament entry (it consumes and produces preparations) or a neighbour
    histograms: tuple = ()  # keys that are histograms: equal bin for bin, the shorter one zero beyond its end (test_game_stats_gpu._eq)


def _plain(e, p, **kw):
    lead, base = _lead(p)
    return e.tournament(*lead, **base, **kw)


def _columns(e, p, async_rows=False):
    lead, base = _lead(p)
    table, k, _, lo, hi = lead
    S, n_sh = len(table), hi - lo
    from farkle_ii_amd.backend import row_columns_bytes

    seeds = {"shuffle_seeds": np.zeros(n_sh, dtype=np.uint32), "game_seeds": np.zeros(n_sh * (S // k), dtype=np.uint32)}
    kw = {}
    if async_rows:  # the copy is still in flight when the call returns: a page-locked buffer of the engine, read after rows_wait
        kw = dict(async_rows=True, columns_out=e.pinned_empty(n_sh * row_columns_bytes(k, S // k), np.uint8))
    out = e.tournament_columns(*lead, ids_for(S), shuffle_seeds_out=seeds["shuffle_seeds"], game_seeds_out=seeds["game_seeds"], **base, **kw)
    # an image is rounded up to a multiple of 64 bytes (include/farkle_hip.h): what lies behind its last column is not part of it
    defined = (4 * (4 + 13 * k) + 2 + k) * (S // k)
    return {**out, **seeds, "columns": out["columns"][:, :defined]}


def _lags(e, p):
    lead, base = _lead(p)
    return e.tournament_lags(*lead, LAGS, **base)


def _matchups(e, p):
    lead, base = _lead(p)
    return e.tournament_matchups(*lead, LAGS, ids_for(len(lead[0])), 12, **base)


def _game_stats(e, p, **kw):
    lead, base = _lead(p)
    return e.tournament_game_stats(*lead, rare_target_score=p["target"], shuffles_per_batch=8, **base, **kw)


def _rare(e, p):
    lead, base = _lead(p)
    return e.tournament_rare_events(*lead, rare_target_score=p["target"], thresholds=(500, 1000), **base)


def _seat_counts(e, p):
    lead, base = _lead(p)
    return e.tournament_seat_counts(*lead, shuffles_per_batch=8, strategy_ids=ids_for(len(lead[0])), want_mirrored=p["k"] == 2, **base)


def _game_list(p, n):
    """n games of (purpose 10, root, k) with seats 0 .. k - 1 of the table, as test_state_store_gpu plays them between two calls."""
    k = p["k"]
    coords = make_coords(10, p["root"], k, 0, 0, 0, np.arange(p["lo"], p["lo"] + n, dtype=np.uint64))
    seats = (np.arange(n, dtype=np.int32)[:, None] * 3 + np.arange(k, dtype=np.int32)[None, :] * 5) % len(tables()[p["table"]])
    return coords, tables()[p["table"]], seats.astype(np.int32), k


def _play_games(e, p):
    return {"rows": e.play_games(*_game_list(p, 50), target_score=p["target"], max_rounds=p["rounds"])}


def _trace(e, p):
    rows, begin, events = e.trace_games(*_game_list(p, 6), target_score=p["target"], max_rounds=p["rounds"])
    return {"rows": rows, "begin": begin, "events": events}


def _h2h_blocks(e, p):
    t = tables()[p["table"]]
    n = 24
    seats = np.stack([t[[(5 * b) % len(t), (7 * b + 3) % len(t)]] for b in range(n)])
    ov = make_overrides([(p["root"], 3, 1, 0, 2)])
    return {"states": e.h2h_blocks(seats, p["root"], np.arange(n) // 2, np.arange(n) % 2, 6, 12, target_score=p["target"], max_rounds=24,
                                   overrides=ov)}


def _rr_table(p):
    return tables()[p["table"]][3:11].copy()


def _round_robin(e, p):
    states, summary = e.h2h_round_robin(_rr_table(p), p["root"], 5, 10, target_score=p["target"], max_rounds=24)
    return {"states": states, "summary": summary}


def _round_robin_resident(e, p):
    e.rr_counts_reset()
    try:
        return {"summary": e.h2h_round_robin_resident(_rr_table(p), p["root"], 5, 10, target_score=p["target"], max_rounds=24)}
    finally:
        e.rr_counts_reset()  # (the accumulator is another test module's subject: none is left behind)


def _census(e, p):
    lead, base = _lead(p)
    table, k, root, lo, _ = lead
    return e.tournament_census(table, k, root, lo, lo + 3, turn_bins=16, **base)


def _seeds(e, p):
    table, k, lo, hi = tables()[p["table"]], p["k"], p["lo"], p["hi"]
    idx = np.arange(lo, hi, dtype=np.uint64)
    return {"game_seeds": e.game_seeds(102, p["root"], k, lo, hi, len(table) // k),
            "shuffle_seeds": e.coordinate_seeds(make_coords(100, p["root"], k, idx), want32=True)[0]}


def _perm_from_draws(e, p):
    S = len(tables()[p["table"]])
    draws = np.array([perm_stage_cases.literal_draws(p["root"], p["k"], s, S) for s in range(p["lo"], p["lo"] + 5)], dtype=np.uint16)
    return {"chains": e.debug_perm_from_draws(S, draws, 1), "chain_free": e.debug_perm_from_draws(S, draws, 2)}


_GS = tuple(f"game_stats.{n}" for n in GAME_STAT_NAMES)
_GS_H = tuple(f"game_stats.{n}" for n in GAME_STAT_NAMES if n not in ("strategy_counts", "game_counts"))
_RARE = ("rare_events.strategy_second", "rare_events.game_second", "rare_events.events", "rare_events.event_head", "rare_events.event_seats")

KINDS = {
    "plain": Kind(_plain, ("tally",), True),
    "plain_batches": Kind(lambda e, p: _plain(e, p, shuffles_per_batch=8), ("tally",), True),
    "rows": Kind(lambda e, p: _plain(e, p, want_rows=True), ("tally", "rows"), True),
    "seat_stats": Kind(lambda e, p: _plain(e, p, want_seat_stats=True, shuffles_per_batch=8), ("tally", "seat_stats", "seat_ratio_sums"), True),
    "columns_seeds": Kind(_columns, ("tally", "columns", "shuffle_seeds", "game_seeds"), True),
    "columns_async": Kind(lambda e, p: _columns(e, p, async_rows=True), ("tally", "columns", "shuffle_seeds", "game_seeds"), True),
    "lags": Kind(_lags, ("tally", "lag_sums", "lag_head", "lag_tail", "n_shuffles"), True),
    "matchups": Kind(_matchups, ("tally", "lag_sums", "lag_head", "lag_tail", "n_shuffles", "matchups.digest", "matchups.seats", "matchups.rounds"), True),
    "game_stats": Kind(_game_stats, ("tally",) + _GS, True, _GS_H),
    "game_stats_seats": Kind(lambda e, p: _game_stats(e, p, want_seat_stats=True), ("tally", "seat_stats", "seat_ratio_sums") + _GS, True, _GS_H),
    "rare_events": Kind(_rare, ("tally",) + _GS + _RARE, True, _GS_H + _RARE[:2]),
    "seat_counts": Kind(_seat_counts, ("tally", "seat_counts", "pair_index", "pair_sums"), True),  # mirrored pairs at k = 2
    # neighbours: they use the context between a hint and its use
    "play_games": Kind(_play_games, ("rows",), False),
    "h2h_blocks": Kind(_h2h_blocks, ("states",), False),
    "round_robin": Kind(_round_robin, ("states", "summary"), False),
    "round_robin_resident": Kind(_round_robin_resident, ("summary",), False),
    "census": Kind(_census, tuple(CENSUS_TABLES), False),
    "trace_games": Kind(_trace, ("rows", "begin", "events"), False),
    "seeds": Kind(_seeds, ("game_seeds", "shuffle_seeds"), False),
    "perm_from_draws": Kind(_perm_from_draws, ("chains", "chain_free"), False),
}
TOURNAMENT_KINDS = tuple(n for n, kd in KINDS.items() if kd.tournament)
NEIGHBOUR_KINDS = tuple(n for n, kd in KINDS.items() if not kd.tournament)


# ---------------------------------------------------------------------------------------------------------------- the CPU engine
class CombinedCpuEngine(rare_events_engine_stub.Engine, seat_analysis_engine_stub.Engine, matchup_engine_stub.Engine, census_engine_stub.Engine,
                        round_robin_engine_stub.Engine):
    """Every CPU stub of the suite in one class (they share ``oracle_engine_stub.Engine``; the trace stub is held, not inherited: its
    ``calls`` counter and the rare-events stub's ``calls`` list are one attribute name), plus the plain statements of the entries no
    stub has: the resident round robin (its summary is the round robin's), the two fingerprint entries (``farkle_ii_amd.random``) and
    the permutation probe (``perm_stage_cases.literal_fisher_yates``)."""

    def __init__(self, device: int = 0):
        super().__init__(device)
        self._trace = trace_engine_stub.TraceEngineStub()

    def trace_games(self, coords, table, seat_strategy, k, target_score=10_000, max_rounds=200):
        return self._trace.trace_games(coords, table, seat_strategy, k, target_score, max_rounds)

    def timing(self) -> dict:
        return {**super().timing(), "prefetched_chunks": 0}

    def rr_counts_reset(self) -> None:
        pass

    def h2h_round_robin_resident(self, table, root_seed, target, max_attempts, pair_begin=0, pair_end=None, target_score=10_000, max_rounds=200,
                                 summary=None, family_pair_count=None):
        return self.h2h_round_robin(table, root_seed, target, max_attempts, pair_begin, pair_end, target_score, max_rounds, summary)[1]

    def coordinate_seeds(self, coords, want32=True, want64=False):
        from farkle_ii_amd import random as urandom

        c = np.asarray(coords)
        kw = dict(root_seed=c["root_seed"], k=c["k"], shuffle_index=c["shuffle_index"], pair_id=c["pair_id"], order=c["order"],
                  game_index=c["game_index"], seat_index=c["seat_index"], replicate_index=c["replicate_index"])
        purposes = np.unique(c["purpose"])
        assert len(purposes) == 1
        return (urandom.coordinate_seeds(int(purposes[0]), dtype=np.uint32, **kw) if want32 else None,
                urandom.coordinate_seeds(int(purposes[0]), dtype=np.uint64, **kw) if want64 else None)

    def game_seeds(self, purpose, root_seed, k, shuffle_begin, shuffle_end, games_per_shuffle):
        from farkle_ii_amd import random as urandom

        sh = np.arange(shuffle_begin, shuffle_end, dtype=np.uint64)
        gps = int(games_per_shuffle)
        out = urandom.coordinate_seeds(int(purpose), root_seed=root_seed, k=k, shuffle_index=np.repeat(sh, gps),
                                       game_index=np.tile(np.arange(gps, dtype=np.uint64), len(sh)), dtype=np.uint32)
        return out.reshape(len(sh), gps)

    def debug_perm_from_draws(self, S, draws, path, out=None, n_sh=None):
        return np.stack([perm_stage_cases.literal_fisher_yates(S, [int(v) for v in row]) for row in np.asarray(draws)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- the driver
def _flat(result: dict, prefix: str = "") -> dict:
    out = {}
    for key, value in result.items():
        if isinstance(value, dict):
            out.update(_flat(value, f"{prefix}{key}."))
        else:
            out[prefix + key] = value
    return out


def canonical(value, histogram: bool = False):
    """What two results are equal by.  Integer arrays: shape and values (the stubs and the engine may hold them in different widths);
    structured arrays (rows, events) and float arrays (``seat_ratio_sums``: bit for bit): dtype, shape and bytes; histograms: the bins
    up to the last non-zero one of any row."""
    if value is None:
        return None
    if isinstance(value, (int, np.integer)):
        return int(value)
    a = np.ascontiguousarray(value)
    if a.dtype.kind in "iub":
        if histogram:
            used = np.flatnonzero(a.reshape(-1, a.shape[-1]).any(axis=0))
            a = np.ascontiguousarray(a[..., :int(used[-1]) + 1 if len(used) else 0])
        wide = a.astype(np.uint64) if a.dtype.kind in "ub" else a.astype(np.int64).view(np.uint64)
        return ("int", a.shape, wide.tobytes())
    return (str(a.dtype), a.shape, a.tobytes())


def _values(kind: str, result: dict) -> dict:
    flat = _flat(result)
    kd = KINDS[kind]
    return {key: canonical(flat[key], key in kd.histograms) for key in kd.keys}


def run(engine, steps) -> list:
    """Executes the steps on ``engine``.  One record per step: None for hints and options; for a call ``{"kind", "values": {key:
    canonical value}, "timing": the engine's timing() right after the call}``.  The images of an async column call are awaited — and
    read — one call late (or at the end of the list)."""
    records = [None] * len(steps)
    pending = None  # (record index, kind, result) of an async column call whose images have not been awaited

    def settle():
        nonlocal pending
        if pending is not None:
            index, kind, result = pending
            engine.rows_wait(result["rows_event"])
            records[index]["values"] = _values(kind, result)
            pending = None

    for i, step in enumerate(steps):
        if step[0] == "hint":
            engine.hint_next(step[1], step[2], need_state=bool(step[3]))
        elif step[0] == "option":
            engine.set_option(step[1], step[2])
        elif step[0] == "call":
            kind, params = step[1], dict(step[2])
            result = KINDS[kind].call(engine, params)
            records[i] = {"kind": kind, "timing": dict(engine.timing())}
            settle()  # the images of the async call in front of this one: awaited one call late
            if kind == "columns_async":
                pending = (i, kind, result)
            else:
                records[i]["values"] = _values(kind, result)
        else:
            raise ValueError(f"unknown step {step!r}")
    settle()
    return records


_EXPECTED: dict = {}


def expected(kind: str, params: tuple) -> dict:
    """The call made alone on a fresh combined CPU engine."""
    key = (kind, params)
    if key not in _EXPECTED:
        steps = [("call", kind, params)]
        _EXPECTED[key] = run(CombinedCpuEngine(), steps)[0]["values"]
    return _EXPECTED[key]


def mismatches(name: str, steps, records) -> list:
    """``(step index, message)`` of every call step whose record differs from its expectation: the sequence, the step index, the step
    itself and the first differing key."""
    out = []
    for i, (step, rec) in enumerate(zip(steps, records)):
        if step[0] != "call":
            continue
        want = expected(step[1], step[2])
        got = rec["values"]
        assert got.keys() == want.keys()
        for key in want:
            if got[key] != want[key]:
                out.append((i, f"{name}: step {i} {_show(step)}: {key} differs"))
                break
    return out


def _show(step) -> str:
    if step[0] != "call":
        return repr(step)
    p = dict(step[2])
    return f"{step[1]}({p['table']}, k={p['k']}, root={p['root']}, {p['lo']}..{p['hi']}, target={p['target']}, rounds={p['rounds']}, ov={p['ov']}, copy={p['copy']})"


# -------------------------------------------------------------------------------------------------------------------- sequences
@dataclass
class Seq:
    """One scripted sequence.  ``checks``: ``(step index, tag)`` — ``"consumer"``: the call a right hint was made for (of the
    sequences that share ``family``, i.e. differ in ``need_state`` only, at least one consumes its preparation when the pipeline is
    on); ``"all_chunks"``: the same for a multi-chunk call (every chunk of it prefetched); ``"wrong"``: a call no preparation exists
    for (it consumes none); ``"chunks"``: the call plays in at least five chunks; ``"chunks3"``: in at least three (a first, a middle and a last one); ``"observe"``:
    reported only."""
    name: str
    steps: list
    checks: list = field(default_factory=list)
    family: tuple = ()
    group: str = ""
    head: int = 0  # the steps in front of the sequence proper (``_head``)


# Shuffle ranges of 24 to 64 shuffles (F: 8), begins on multiples of 8.  A is the producing call's and B the hinted one's: B is the
# shorter, because a preparation is cut to the length of the call that makes it (tournament_run_impl clamps its chunk length to its own
# range before it describes the hinted chunk), so a hinted range LONGER than the producer's is never found — see LONG_B.
A, B, C, D, E, F = (8, 48), (48, 72), (80, 120), (120, 144), (144, 208), (0, 8)
LONG_B = (48, 112)  # 64 shuffles behind A's 40: a right hint by the documentation; results only, and its prefetched_chunks is reported
# 70 shuffles of the 1 024-strategy table under chunk_bytes = SMALL.  A chunk holds 2 S bytes of permutation per shuffle and, per game,
# k x (state record + 16) + 8 bytes and more (game_workspace_bytes).  A rows call has 48-byte state records and 4 + 28 k bytes of row:
# at least 196 bytes per game at k = 2 and 380 at k = 4, ten shuffles per chunk at most, seven chunks.  A plain call with 18-byte records
# holds 2 S + S / k x (34 k + 8) bytes per shuffle at least, 25 or 26 shuffles per chunk at most: three chunks at least, and the
# result records it may need on top only make it more (observed: four).
WIDE_A, WIDE_B = (0, 70), (72, 142)


def _chunks(kind: str) -> str:
    return "chunks" if kind == "rows" else "chunks3"


def _head(pipeline: int) -> list:
    """What every scripted sequence begins with: the pipeline option, and one call with the OTHER table of 64.  The table change voids
    whatever an earlier sequence left prepared (a preparation nobody consumed stays valid for any later call it describes, with the
    pipeline on or off), so that the conditions on ``prefetched_chunks`` speak about this sequence's hint alone."""
    return [("option", "pipeline", pipeline), ("call", "plain", P(table="g64b", lo=F[0], hi=F[1]))]


def _seq(name: str, pipeline: int, body: list, checks: list, family: tuple, group: str) -> "Seq":
    """``checks`` index the body; the head goes in front."""
    head = _head(pipeline)
    return Seq(name, head + body, [(len(head) + i, tag) for i, tag in checks], family, group, len(head))


def _r(rng, **kw) -> tuple:
    return P(lo=rng[0], hi=rng[1], **kw)


def group_a(k: int, pipeline: int) -> list:
    """Right hint, every consumer."""
    out = []
    for kind in TOURNAMENT_KINDS:
        for ns in (False, True):
            body = [("hint", *B, ns), ("call", "plain", _r(A, k=k)), ("call", kind, _r(B, k=k))]
            out.append(_seq(f"a/{kind}/k{k}/state{int(ns)}/p{pipeline}", pipeline, body, [(2, "consumer")], ("a", kind, k), "a"))
    return out


def group_b(k: int, pipeline: int) -> list:
    """Every producer: the call that carries the hint."""
    out = []
    for kind in TOURNAMENT_KINDS:
        for ns in (False, True):
            body = [("hint", *B, ns), ("call", kind, _r(A, k=k)), ("call", "plain", _r(B, k=k))]
            out.append(_seq(f"b/{kind}/k{k}/state{int(ns)}/p{pipeline}", pipeline, body, [(2, "consumer")], ("b", kind, k), "b"))
    return out


WRONG_VARIANTS = ("other_range", "same_begin_other_end", "other_root", "other_k", "other_table", "longest_first", "chunk_bytes")
STILL_VARIANTS = ("fresh_copy", "other_limits")
OBSERVED_VARIANTS = ("hinted_longer",)  # compared with the CPU statement like every call; no condition on prefetched_chunks


def group_c(k: int, pipeline: int) -> list:
    """Wrong hints: the call after the hinted one differs from the hint in exactly one thing; then the hinted call after all.  And the
    two variants that must still consume the preparation."""
    out = []
    for ns in (False, True):
        def seq(variant, steps, checks, family=()):
            out.append(_seq(f"c/{variant}/k{k}/state{int(ns)}/p{pipeline}", pipeline, steps, checks, family, "c"))

        lead = [("hint", *B, ns), ("call", "plain", _r(A, k=k))]
        after_all = ("call", "plain", _r(B, k=k))
        for variant, wrong in (("other_range", _r(C, k=k)), ("same_begin_other_end", P(k=k, lo=B[0], hi=B[1] - 8)), ("other_root", _r(B, k=k, root=43)),
                               ("other_k", _r(B, k=6 - k)), ("other_table", _r(B, k=k, table="g64b"))):
            seq(variant, lead + [("call", "plain", wrong), after_all], [(2, "wrong")])
        seq("longest_first", lead + [("option", "longest_first", 0), ("call", "plain", _r(B, k=k)), ("option", "longest_first", 1), after_all],
            [(3, "wrong")])
        wide = dict(k=k, table="g1024")
        seq("chunk_bytes", [("option", "chunk_bytes", SMALL), ("hint", *WIDE_B, ns), ("call", "plain", _r(WIDE_A, **wide)), ("option", "chunk_bytes", BIG),
                            ("call", "plain", _r(WIDE_B, **wide)), ("option", "chunk_bytes", SMALL), ("call", "plain", _r(WIDE_B, **wide)),
                            ("option", "chunk_bytes", BIG)], [(2, _chunks("plain")), (4, "wrong"), (6, _chunks("plain"))])
        seq("hinted_longer", [("hint", *LONG_B, ns), ("call", "plain", _r(A, k=k)), ("call", "plain", _r(LONG_B, k=k))], [(2, "observe")],
            ("c", "hinted_longer", k))
        seq("fresh_copy", lead + [("call", "plain", _r(B, k=k, copy=True))], [(2, "consumer")], ("c", "fresh_copy", k))
        seq("other_limits", lead + [("call", "plain", _r(B, k=k, target=2000, rounds=6, ov=((2, 3, 1), (5, 0, 3), (7, 2, 0))))], [(2, "consumer")],
            ("c", "other_limits", k))
    return out


def group_d(k: int, pipeline: int) -> list:
    """Neighbours between a hint and its use: one, then two in a row; the hinted call is a plain call (4-dword seeding at k = 2) or a
    rows call (state records)."""
    out = []
    pairs = list(zip(NEIGHBOUR_KINDS, NEIGHBOUR_KINDS[1:] + NEIGHBOUR_KINDS[:1]))
    for consumer, ns in (("plain", False), ("rows", True)):
        for between in [(n,) for n in NEIGHBOUR_KINDS] + pairs:
            body = [("hint", *B, ns), ("call", "plain", _r(A, k=k))]
            body += [("call", n, _r(C, k=k)) for n in between] + [("call", consumer, _r(B, k=k))]
            out.append(_seq(f"d/{'+'.join(between)}/{consumer}/k{k}/p{pipeline}", pipeline, body, [], (), "d"))
    return out


def group_e(k: int, pipeline: int) -> list:
    """Multi-chunk: the hinting and the hinted call both play in several chunks; then the hinted call is a rows call, whose chunks
    are shorter than those the plain call prepared for."""
    out = []
    wide = dict(k=k, table="g1024")
    for ns in (False, True):
        body = [("option", "chunk_bytes", SMALL), ("hint", *WIDE_B, ns), ("call", "plain", _r(WIDE_A, **wide)),
                ("call", "plain", _r(WIDE_B, **wide)), ("hint", *WIDE_A, ns), ("call", "plain", _r(WIDE_B, **wide)),
                ("call", "rows", _r(WIDE_A, **wide)), ("option", "chunk_bytes", BIG)]
        out.append(_seq(f"e/k{k}/state{int(ns)}/p{pipeline}", pipeline, body,
                        [(2, _chunks("plain")), (3, _chunks("plain")), (3, "all_chunks"), (5, _chunks("plain")), (6, _chunks("rows"))], ("e", k), "e"))
    return out


def group_f(k: int, pipeline: int) -> list:
    """A hint and nothing after it: four calls over ranges nobody hinted.  The orphaned preparation is overwritten or kept, never used."""
    out = []
    for ns in (False, True):
        body = [("hint", *B, ns), ("call", "plain", _r(A, k=k)), ("call", "rows", _r(C, k=k)), ("call", "lags", _r(D, k=k)),
                ("call", "game_stats", _r(E, k=k)), ("call", "seat_counts", _r(F, k=k)), ("call", "plain", _r(B, k=k))]
        out.append(_seq(f"f/k{k}/state{int(ns)}/p{pipeline}", pipeline, body, [(i, "wrong") for i in (2, 3, 4, 5)], (), "f"))
    return out


def group_g(k: int, pipeline: int) -> list:
    """Async column images between sync rows calls and plain calls: the two device row buffers alternate over the chunks of a rows call
    (``rows_chunk_games`` = 300: three, four or five chunks per call here) and, in async mode, over calls; the four rows events turn over."""
    c = lambda kind, rng: ("call", kind, _r(rng, k=k))  # noqa: E731
    body = [
        ("option", "rows_chunk_games", 300),
        c("columns_async", A), c("rows", B), c("columns_async", C), c("plain", D), c("plain", A), c("columns_async", D), c("rows", A), c("rows", C),
        c("columns_async", B), c("columns_async", A), ("hint", *C, True), c("columns_async", D), c("columns_async", C), c("rows", D), c("plain", B),
        c("columns_async", F), c("columns_seeds", A), c("columns_async", E), c("seat_stats", B), c("columns_async", B),
        ("option", "rows_chunk_games", 4_000_000),
        c("columns_async", A), c("rows", B), c("columns_async", B), c("columns_async", C),
    ]
    return [_seq(f"g/k{k}/p{pipeline}", pipeline, body, [], (), "g")]


WALK_SEEDS = (20261, 20262, 20263)
WALK_RANGES = (A, B, C, D, F)


def _kind_tour(rng: random.Random) -> list:
    """A closed walk over the tournament kinds that takes every ordered pair (self-pairs included) once: an Euler circuit of the
    complete directed graph, its edges taken in random order (Hierholzer)."""
    left = {a: rng.sample(TOURNAMENT_KINDS, len(TOURNAMENT_KINDS)) for a in TOURNAMENT_KINDS}
    stack, tour = [rng.choice(TOURNAMENT_KINDS)], []
    while stack:
        if left[stack[-1]]:
            stack.append(left[stack[-1]].pop())
        else:
            tour.append(stack.pop())
    return tour[::-1]


@lru_cache(maxsize=None)
def walks(pipeline: int = 1) -> tuple:
    """Three seeded walks.  The kinds follow one random tour through every ordered pair of tournament kinds, cut into three parts
    that overlap by one call; k, table (two tables of 64), range, hint (right, wrong or none), ``need_state`` and the places of the
    neighbours are drawn at random.  A neighbour is followed by the kind in front of it once more, so that no pair of the tour is lost."""
    tour = _kind_tour(random.Random(WALK_SEEDS[0]))
    third = (len(tour) + 2) // 3
    deck = itertools.cycle(random.Random(WALK_SEEDS[0]).sample(NEIGHBOUR_KINDS, len(NEIGHBOUR_KINDS)))  # every neighbour gets its turn
    out = []
    for w, seed in enumerate(WALK_SEEDS):
        rng = random.Random(seed)
        kinds = tour[w * third:(w + 1) * third + 1]
        calls, k, table = [], rng.choice((2, 4)), "g64"
        for kind in kinds:
            if rng.random() < 0.3:
                k = 6 - k
            if rng.random() < 0.2:
                table = "g64b" if table == "g64" else "g64"
            params = _r(rng.choice(WALK_RANGES), k=k, table=table)
            calls.append(("call", kind, params))
            if rng.random() < 0.18:
                calls.append(("call", next(deck), _r(rng.choice(WALK_RANGES), k=k, table=table)))
                calls.append(("call", kind, _r(rng.choice(WALK_RANGES), k=k, table=table)))
        steps = [("option", "pipeline", pipeline)]  # (no table change in front: a walk starts from whatever the context holds)
        for i, call in enumerate(calls):
            nxt = next((c for c in calls[i + 1:] if KINDS[c[1]].tournament), None)
            draw = rng.random()
            if KINDS[call[1]].tournament and nxt is not None and draw < 0.75:
                p = dict(nxt[2])
                lo, hi = (p["lo"], p["hi"]) if draw < 0.5 else rng.choice([r for r in WALK_RANGES if r != (p["lo"], p["hi"])])
                steps.append(("hint", lo, hi, rng.random() < 0.5))
            steps.append(call)
        out.append(Seq(f"h/walk{w}/p{pipeline}", steps, [], (), "h", 1))
    return tuple(out)


GROUPS = {"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e, "f": group_f, "g": group_g}


def perm_split_sequences(pipeline: int) -> list:
    """The draws + chain-free permutation path (``perm_split`` = 2) on the 64-strategy table, instead of a large table: a right hint and
    a wrong one at both k."""
    out = []
    for k in (2, 4):
        body = [("option", "perm_split", 2), ("hint", *B, True), ("call", "plain", _r(A, k=k)), ("call", "rows", _r(B, k=k)),
                ("hint", *D, False), ("call", "plain", _r(B, k=k)), ("call", "plain", _r(C, k=k)), ("call", "plain", _r(D, k=k)),
                ("option", "perm_split", -1)]
        out.append(_seq(f"split/k{k}/p{pipeline}", pipeline, body, [(3, "consumer"), (6, "wrong")], ("split", k), "split"))
    return out


def sequences(group: str, k: int, pipeline: int) -> list:
    if group == "h":
        return list(walks(pipeline))
    return GROUPS[group](k, pipeline)


RESTORE = (("pipeline", 1), ("chunk_bytes", BIG), ("longest_first", 1), ("rows_chunk_games", 4_000_000), ("perm_split", -1))  # the defaults of every option a sequence sets


# ------------------------------------------------------------------------------------------------------- the hint conditions
def hint_violations(seqs, records_of: dict, pipeline: int) -> list:
    """The conditions on ``timing()["prefetched_chunks"]`` that make the hint sequences non-vacuous: ``(sequence name, step index, tag,
    message)`` of every one that does not hold.  ``records_of``: sequence name -> ``run``'s records."""
    out = []
    consumed: dict = {}
    for s in seqs:
        rec = records_of[s.name]
        for index, tag in s.checks:
            t = rec[index]["timing"]
            got, launches = t["prefetched_chunks"], t["play_launches"]
            where = f"{s.name}: step {index} {_show(s.steps[index])}: prefetched_chunks {got}, play_launches {launches}"
            if tag in ("chunks", "chunks3"):
                if launches < (5 if tag == "chunks" else 3):
                    out.append((s.name, index, "chunks", f"{where}: fewer than {'five' if tag == 'chunks' else 'three'} chunks"))
            elif tag == "observe" and pipeline:
                pass
            elif pipeline == 0:
                if got != 0:
                    out.append((s.name, index, tag, f"{where}: the pipeline is off"))
            elif tag == "wrong":
                if got != 0:
                    out.append((s.name, index, tag, f"{where}: a call nothing was prepared for consumed a preparation"))
            else:  # "consumer": at least one chunk; "all_chunks": every chunk of the call
                ok = got >= 1 if tag == "consumer" else got == launches
                consumed.setdefault((s.family, tag), []).append((ok, s.name, index, where))
    for (family, tag), seen in consumed.items():
        if not any(ok for ok, *_ in seen):
            out.append((seen[0][1], seen[0][2], tag, f"{family}: no need_state value had its preparation consumed: " + "; ".join(w[3] for w in seen)))
    return out


def consumed_table(seqs, records_of: dict) -> dict:
    """``{family: {need_state: prefetched_chunks of the consuming call}}`` of the sequences with a ``"consumer"`` check (the observed
    ``need_state`` table of DESIGN "What outlives a call")."""
    out: dict = {}
    for s in seqs:
        for index, tag in s.checks:
            if tag in ("consumer", "observe"):
                ns = next(step[3] for step in s.steps if step[0] == "hint")
                out.setdefault(s.family, {})[bool(ns)] = records_of[s.name][index]["timing"]["prefetched_chunks"]
    return out


# -------------------------------------------------------------------------------------------------------- the detector engines
_TOURNAMENT_METHODS = ("tournament", "tournament_columns", "tournament_lags", "tournament_matchups", "tournament_game_stats", "tournament_rare_events",
                       "tournament_seat_counts")
_NEIGHBOUR_METHODS = ("play_games", "h2h_blocks", "h2h_round_robin", "h2h_round_robin_resident", "tournament_census", "trace_games", "game_seeds",
                      "coordinate_seeds", "debug_perm_from_draws")


class StaleEngine:
    """A deliberately WRONG engine: after a hint, the call behind the hinted one's producer is answered with the prepared range
    whenever its begin shuffle matches the hint's (``match="begin"``) or whatever it asks for (``match="any"``) — end, root, k, table,
    ``need_state``, target and rounds are those of the preparation, i.e. of the producing call.  It reports the stale
    answer as a consumed preparation in ``timing()``."""

    def __init__(self, match: str = "begin"):
        self._inner = CombinedCpuEngine()
        self._match = match
        self._hint = None      # (lo, hi) of a hint no call has taken yet
        self._prepared = None  # (table, k, root, lo, hi, target_score, max_rounds) of the preparation
        self._stale = 0

    def hint_next(self, lo, hi, need_state=False):
        self._hint = (lo, hi)

    def timing(self):
        return {**self._inner.timing(), "prefetched_chunks": self._stale}

    def __getattr__(self, name):
        inner = getattr(self._inner, name)
        if name not in _TOURNAMENT_METHODS:
            return inner

        def call(table, k, root, lo, hi, *args, **kw):
            self._stale = 0
            lead = (table, k, root, lo, hi)
            prepared, self._prepared = self._prepared, None
            if prepared is not None and (self._match == "any" or lo == prepared[3]):
                lead = prepared[:5]
                kw = {**kw, "target_score": prepared[5], "max_rounds": prepared[6]}
                self._stale = 1
            elif self._hint is not None:
                self._prepared = (table, k, root, *self._hint, kw.get("target_score", 10_000), kw.get("max_rounds", 200))
            self._hint = None
            return inner(*lead, *args, **kw)

        return call


class ResidueEngine:
    """A deliberately WRONG engine: the first tournament call after a neighbour call returns a tally with one cell off."""

    def __init__(self):
        self._inner = CombinedCpuEngine()
        self._dirty = False

    def __getattr__(self, name):
        inner = getattr(self._inner, name)
        if name in _NEIGHBOUR_METHODS:
            def neighbour(*args, **kw):
                self._dirty = True
                return inner(*args, **kw)
            return neighbour
        if name in _TOURNAMENT_METHODS:
            def call(*args, **kw):
                out = inner(*args, **kw)
                if self._dirty:
                    out["tally"] = out["tally"].copy()
                    out["tally"].reshape(-1)[3] += 1
                    self._dirty = False
                return out
            return call
        return inner
