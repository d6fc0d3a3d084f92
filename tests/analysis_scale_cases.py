"""TEST INFRASTRUCTURE ONLY — the game-stats, rare-event and seat-analysis post-passes at the production table (5 160 strategies)
and at launches large enough to leave the regimes the small GPU tests stay in: permutation images in blocks of fewer than 512
shuffles (S > 160), an event scan of several waves (> 16 384 games) and of two tiles (> 262 144 games), a second trip of the
record kernels' grid-stride loop (> 524 288 games), seat counts beyond one workgroup, more than 65 536 mirrored pairs and ID ranks
beyond six bits.  The case table, each case's expected result (the oracle-backed stubs, computed once per process) and the
preconditions on that result which prove the case reaches its regime."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from rare_events_engine_stub import Engine as RareStub
from seat_analysis_engine_stub import Engine as SeatStub
from test_rng_matchups_gpu import _odd_ids

from farkle_ii_amd import game_stats as gs
from farkle_ii_amd import rare_events as rev

GRID = 5160
RARE_ROOT, RARE_BEGIN = 9, 7  # (a call that does not begin at shuffle 0: event shuffles count from the call's first)
SEAT_ROOT = 3
MIXED = dict(rare_target_score=1500, thresholds=(100, 300))

# name -> k, shuffles, arguments beside target_score, the game id some event must lie at or beyond, whether every completed game
# is an event.  Games = shuffles * (5 160 // k).  What the reference result holds (test_analysis_scale_cpu.py prints it):
#   slots_multiwave   24 253 events, 17 414 of them multi alone, 931 safety-limit games
#   two_tiles_mixed   62 263 events, 865 of them at game id >= 262 144
#   two_tiles_dense   263 288 events = completed games, 3 562 at id >= 262 144
#   two_tiles_k3      102 213 events, 1 009 at id >= 262 144
#   grid_stride       100 853 events, 861 at id >= 524 288, 118 859 safety-limit games
#   hot_cold_k12      12 881 events, 8 237 of them multi alone, 594 at id >= 16 384, no safety-limit game
RARE_CASES = {
    "slots_multiwave": dict(k=2, n_sh=40, kw=MIXED, beyond=16_384, dense=False),       # 103 200 games
    "two_tiles_mixed": dict(k=2, n_sh=103, kw=MIXED, beyond=262_144, dense=False),     # 265 740
    "two_tiles_dense": dict(k=2, n_sh=103, kw=dict(rare_target_score=10 ** 6, thresholds=(2 ** 31 - 1,)), beyond=262_144, dense=True),
    "two_tiles_k3": dict(k=3, n_sh=154, kw=MIXED, beyond=262_144, dense=False),        # 264 880
    "grid_stride": dict(k=2, n_sh=205, kw=dict(rare_target_score=1500, thresholds=(100,), max_rounds=6), beyond=524_288, dense=False),  # 528 900
    "hot_cold_k12": dict(k=12, n_sh=40, kw=MIXED, beyond=16_384, dense=False),         # 17 200
}

# name -> S, k, shuffle range, shuffles per batch, arguments beside target_score.  The reference result:
#   pairs_5160   102 832 pairs, 64 of them with paired > 0, 901 safety-limit games
#   pairs_300    44 756 pairs, largest paired 7, 22 409 non-zero differences, 16 746 safety-limit games, unpaired 67 761 / 67 867
#   counts_k5    41 280 games in three batches (16 + 16 + 8 shuffles), one safety-limit game
SEAT_CASES = {
    "pairs_5160": dict(S=5160, k=2, begin=32, end=72, spb=16, mirrored=True, kw=dict(pair_capacity=10 ** 6)),  # 103 200 games
    "pairs_300": dict(S=300, k=2, begin=0, end=1800, spb=600, mirrored=True, kw=dict(max_rounds=8)),           # 270 000
    "counts_k5": dict(S=5160, k=5, begin=32, end=72, spb=16, mirrored=False, kw={}),                           # 41 280
}


@lru_cache(maxsize=None)
def table(S: int, k: int) -> np.ndarray:
    """The first S strategies of the production grid, cut to a multiple of k."""
    from tools.time_config import table_for

    t = table_for(GRID)[:S]
    t = t[:len(t) // k * k].copy()
    t.setflags(write=False)
    return t


def ids(S: int) -> np.ndarray:
    """Unique IDs whose order is not the table's: the production table reversed, the smaller one scattered."""
    return np.arange(S, dtype=np.int32)[::-1].copy() if S == GRID else _odd_ids(S)


# ---------------------------------------------------------------------------------------------------------- rare events
def rare_games(name: str) -> int:
    c = RARE_CASES[name]
    return c["n_sh"] * (len(table(GRID, c["k"])) // c["k"])


def rare_call(engine, name: str, **extra) -> dict:
    c = RARE_CASES[name]
    kw = dict(c["kw"], target_score=2000, **extra)
    return engine.tournament_rare_events(table(GRID, c["k"]), c["k"], RARE_ROOT, RARE_BEGIN, RARE_BEGIN + c["n_sh"], **kw)


def game_stats_call(engine, name: str) -> dict:
    c = RARE_CASES[name]
    kw = {key: v for key, v in c["kw"].items() if key != "thresholds"}
    return engine.tournament_game_stats(table(GRID, c["k"]), c["k"], RARE_ROOT, RARE_BEGIN, RARE_BEGIN + c["n_sh"], target_score=2000, **kw)


@lru_cache(maxsize=None)
def rare_want(name: str) -> dict:
    """The stub's result with room for every event (never changed by a test)."""
    return rare_call(RareStub(), name, event_capacity=10 ** 6)


def event_ids(res: dict, name: str) -> np.ndarray:
    """The game id (shuffle of the call * games per shuffle + game) of every event."""
    c = RARE_CASES[name]
    f = rev.event_fields(res["rare_events"]["event_head"])
    return f["shuffle"] * (len(table(GRID, c["k"])) // c["k"]) + f["game"]


def rare_figures(name: str) -> dict:
    """What the reference result holds, for the preconditions and the record."""
    want, c = rare_want(name), RARE_CASES[name]
    f = rev.event_fields(want["rare_events"]["event_head"])
    counts = want["game_stats"]["game_counts"]
    return {"games": rare_games(name), "events": int(want["rare_events"]["events"]), "multi_only": int((f["multi"] & (f["mask"] == 0)).sum()),
            "beyond": int((event_ids(want, name) >= c["beyond"]).sum()), "completed": int(counts[gs.COMPLETED]),
            "safety": int(counts[gs.SAFETY]), "spilled": int(want["spilled"])}


def check_rare_preconditions(name: str) -> dict:
    """The reference result reaches the case's regime; -> its figures."""
    c, fig = RARE_CASES[name], rare_figures(name)
    assert fig["games"] > c["beyond"]
    assert fig["events"] > 0
    if c["dense"]:
        assert fig["events"] == fig["completed"]
    else:
        assert fig["events"] < fig["games"]
    assert fig["beyond"] >= 1, f"no event at game id >= {c['beyond']}"
    assert fig["spilled"] == 0
    assert fig["completed"] + fig["safety"] == fig["games"]
    return fig


# -------------------------------------------------------------------------------------------------------- seat analysis
def seat_games(name: str) -> int:
    c = SEAT_CASES[name]
    return (c["end"] - c["begin"]) * (len(table(c["S"], c["k"])) // c["k"])


def seat_call(engine, name: str, **extra) -> dict:
    c = SEAT_CASES[name]
    kw = dict(c["kw"], shuffles_per_batch=c["spb"], target_score=2000, **extra)
    if c["mirrored"]:
        kw.update(strategy_ids=ids(c["S"]), want_mirrored=True)
    return engine.tournament_seat_counts(table(c["S"], c["k"]), c["k"], SEAT_ROOT, c["begin"], c["end"], **kw)


@lru_cache(maxsize=None)
def seat_want(name: str) -> dict:
    return seat_call(SeatStub(), name)


def seat_figures(name: str) -> dict:
    from farkle_ii_amd import seat_analysis as sa

    want = seat_want(name)
    fig = {"games": seat_games(name), "safety": int(want["seat_counts"][..., sa.SAFETY].sum()) // SEAT_CASES[name]["k"]}
    if want["pair_sums"] is not None:
        s = want["pair_sums"]
        fig.update(pairs=len(s), paired_rows=int((s[:, 0] > 0).sum()), paired_max=int(s[:, 0].max()), differences=int((s[:, 1] != 0).sum()),
                   pair_safety=int(s[:, 3].sum()), unpaired=(int(s[:, 4].sum()), int(s[:, 5].sum())))
    return fig


def check_seat_preconditions(name: str) -> dict:
    c, fig = SEAT_CASES[name], seat_figures(name)
    want = seat_want(name)
    assert want["seat_counts"].shape == ((c["end"] - c["begin"] + c["spb"] - 1) // c["spb"], len(table(c["S"], c["k"])), c["k"], 3)
    assert want["seat_counts"][..., 1:].sum() == fig["games"] * c["k"]  # one exposure per seat per game
    if name == "pairs_5160":
        assert fig["pairs"] > 65_536 and fig["paired_rows"] > 0
    if name == "pairs_300":
        assert fig["paired_max"] >= 2 and fig["unpaired"][0] > 0 and fig["unpaired"][1] > 0
        assert fig["differences"] > 0 and fig["pair_safety"] > 0
    return fig
