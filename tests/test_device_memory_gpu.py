"""The context's device buffers: typed, named and owned (csrc/fk_buffers.h).  ``fk_get_option("device_bytes_held")`` is the device
memory the buffers of every live context of this process hold, so it measures what a context leaks without being moved by anybody
else's work on the card.

1. An engine that has made one small call of every entry that allocates gives everything back when it is closed: the figure returns
   exactly to where it was before the engine was created.
2. The same calls made in reverse order on a fresh engine return the same arrays bit for bit (no named buffer serves two roles), and the
   tallies and rows that have a CPU oracle equal it.
3. A call replayed after hipErrorOutOfMemory holds no more than the same call on a roomy engine: the replay frees what it freed before.
"""
from __future__ import annotations

import census_cases
import numpy as np
import performance_bootstrap_cases as pc
import pytest
import root_stability_cases as rc

pytestmark = pytest.mark.gpu

LAGS = (1, 2, 7)
IDS = ((np.arange(12, dtype=np.int64) * 37 + 11) % 257).astype(np.int32)  # unique, not in table order
RANGE = dict(root_seed=42, shuffle_begin=100, shuffle_end=140, shuffles_per_batch=20)  # two batches


def _held(eng) -> int:
    return eng.get_option("device_bytes_held")


def _inputs():
    from farkle_ii_amd.backend import COORD_DTYPE, STRATEGY_DTYPE

    table = np.ascontiguousarray(census_cases.g64()[:12], dtype=STRATEGY_DTYPE)  # twelve strategies: k = 2 and k = 3 both divide them
    coords, mixed, seats = census_cases.two_seat_list(24)
    games = (np.ascontiguousarray(coords, dtype=COORD_DTYPE), np.ascontiguousarray(mixed, dtype=STRATEGY_DTYPE),
             np.ascontiguousarray(seats, dtype=np.int32).reshape(-1))
    return table, games


def _columns(e, t):
    seeds = {"shuffle_seeds": np.zeros(40, dtype=np.uint32), "game_seeds": np.zeros(40 * 6, dtype=np.uint32)}
    out = e.tournament_columns(t, 2, RANGE["root_seed"], RANGE["shuffle_begin"], RANGE["shuffle_end"], IDS, shuffles_per_batch=20,
                               shuffle_seeds_out=seeds["shuffle_seeds"], game_seeds_out=seeds["game_seeds"])
    # an image is rounded up to a multiple of 64 bytes (include/farkle_hip.h); what lies behind its last column is not part of it
    defined = (4 * (4 + 13 * 2) + 2 + 2) * 6
    assert defined <= out["columns"].shape[1] < defined + 64
    return {**out, "columns": out["columns"][:, :defined].copy(), **seeds}


def _matchups(e, t):
    out = e.tournament_matchups(t, 3, 42, 100, 140, LAGS, IDS, 12, shuffles_per_batch=20)
    return {"run": out, "reduce": e.matchup_reduce(out["matchups"], 3, LAGS, 5)}


def _bootstrap(e, t):
    ks, wins, exposures = pc.synthetic(8, 70, {2: 9, 3: 5})
    return e.performance_bootstrap(77, ks, wins, exposures, 3, 40, 10, 0.01, controls=(4,))


def _root_bootstrap(e, t):
    ks, wins, exposures = rc.synthetic(9, 70, {2: 5, 3: 1}, {2: 1, 3: 7})
    return e.root_stability_bootstrap((3, 8), ks, wins, exposures, [0.25, 0.75], 5, 45, 7, want_membership=True, **rc.synthetic_joint(71, 2, 70))


def _round_robin(e, t):
    states, summary = e.h2h_round_robin(t[:4], 42, 5, 10)
    return {"states": states, "summary": summary}


def _entries(games):
    """One small call of every entry that allocates device memory: (name, call(engine, table) -> arrays)."""
    t2 = lambda name, **kw: (name, lambda e, t: getattr(e, name)(t, 2, 42, 100, 140, shuffles_per_batch=20, **kw))  # noqa: E731
    coords, mixed, seats = games
    return [
        ("plain_k2", lambda e, t: e.tournament(t, 2, 42, 100, 140, shuffles_per_batch=20)),
        ("plain_k3", lambda e, t: e.tournament(t, 3, 42, 100, 140, shuffles_per_batch=20)),
        ("rows", lambda e, t: e.tournament(t, 2, 42, 100, 140, shuffles_per_batch=20, want_rows=True)),
        ("columns_seeds", _columns),
        ("seat_stats", lambda e, t: e.tournament(t, 3, 42, 100, 140, shuffles_per_batch=20, want_seat_stats=True, want_seat_ratios=True)),
        ("lags", lambda e, t: e.tournament_lags(t, 2, 42, 100, 140, LAGS, shuffles_per_batch=20)),
        ("matchups", _matchups),
        t2("tournament_game_stats"),
        t2("tournament_rare_events", thresholds=(500, 1000)),
        t2("tournament_seat_counts", strategy_ids=IDS, want_mirrored=True),
        ("play_games", lambda e, t: e.play_games(coords, mixed, seats, 2)),
        ("trace_games", lambda e, t: dict(zip(("rows", "event_begin", "events"), e.trace_games(coords, mixed, seats, 2)))),
        ("census_games", lambda e, t: e.census_games(coords, mixed, seats, 2)),
        ("tournament_census", lambda e, t: e.tournament_census(t, 2, 42, 100, 140, shuffles_per_batch=20)),
        ("h2h", lambda e, t: e.h2h(t[[3, 7]], 42, 5, 0, 20, 40, 40)),
        ("h2h_blocks", lambda e, t: e.h2h_blocks(np.stack([t[[3, 7]], t[[1, 9]]]), 42, [5, 6], [0, 1], 20, 40)),
        ("h2h_round_robin", _round_robin),
        ("performance_bootstrap", _bootstrap),
        ("root_stability_bootstrap", _root_bootstrap),
        ("debug_dice", lambda e, t: dict(zip(("faces", "raw"), e.debug_dice(coords[:8], [6, 3, 1])))),
        ("game_seeds", lambda e, t: e.game_seeds(102, 42, 2, 100, 140, 6)),
    ]


def _flat(value, prefix="") -> dict:
    if isinstance(value, dict):
        out = {}
        for key, v in value.items():
            out.update(_flat(v, f"{prefix}.{key}"))
        return out
    return {prefix: value}


def _run_all(engine, table, entries) -> dict:
    return {name: _flat(call(engine, table), name) for name, call in entries}


@pytest.fixture(scope="module")
def session_engine():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def first_run(session_engine, inputs):
    """Every entry once on a second engine, in order: (results, the figure before the engine, with its buffers, after its close)."""
    from farkle_ii_amd.backend import Engine

    table, games = inputs
    before = _held(session_engine)
    second = Engine(0)
    try:
        results = _run_all(second, table, _entries(games))
        during = _held(session_engine)
    finally:
        second.close()
    return results, before, during, _held(session_engine)


def test_a_destroyed_context_gives_back_everything(first_run):
    _, before, during, after = first_run
    assert during > before  # the engine's buffers were counted while it lived ...
    assert after == before  # ... and every one of them was freed with it


def test_the_same_calls_in_reverse_order_return_the_same_arrays(first_run, inputs):
    import pyoracle as po

    from farkle_ii_amd.backend import Engine

    table, games = inputs
    want = first_run[0]
    with Engine(0) as fresh:
        got = _run_all(fresh, table, list(reversed(_entries(games))))
    assert got.keys() == want.keys()
    for name in want:
        assert got[name].keys() == want[name].keys(), name
        for key, w in want[name].items():
            g = got[name][key]
            if isinstance(w, np.ndarray):
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), key
            else:
                assert g == w, key
    # the CPU oracle of the neighbouring tests (test_memory_gpu.py, test_hip_parity.py): the tallies of both seatings, the rows of the list
    for k, name in ((2, "plain_k2"), (3, "plain_k3")):
        oracle = po.tournament(table.view(po.STRATEGY_DTYPE), k, 42, 100, 140, shuffles_per_batch=20, n_threads=8)["tally"]
        assert np.array_equal(want[name][f"{name}.tally"], oracle), name
    for name, k in (("rows", 2), ("columns_seeds", 2), ("seat_stats", 3), ("lags", 2), ("tournament_game_stats", 2), ("tournament_rare_events", 2),
                    ("tournament_seat_counts", 2)):
        assert want[name][f"{name}.tally"].tobytes() == want[f"plain_k{k}"][f"plain_k{k}.tally"].tobytes(), name
    assert want["matchups"]["matchups.run.tally"].tobytes() == want["plain_k3"]["plain_k3.tally"].tobytes()
    coords, mixed, seats = games
    rows = want["play_games"]["play_games"]
    ref = po.play_games(coords.view(po.COORD_DTYPE), mixed.view(po.STRATEGY_DTYPE), seats.reshape(-1, 2), 2, n_threads=8)
    assert rows.tobytes() == ref.view(rows.dtype).tobytes()
    assert want["trace_games"]["trace_games.rows"].tobytes() == rows.tobytes()


def test_a_replayed_call_holds_no_more_than_a_roomy_one():
    """tests/test_memory_gpu.py's replay (a budget of 2 000 % of what is free with 300 MB left), read through the figure: the replay gives
    its workspace back before it plans again, so what the engine holds afterwards is at most what the same call leaves on a roomy engine."""
    from farkle_ii_amd.backend import Engine
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies, prepare_public_helper_strategies

    table = pack_strategies(prepare_public_helper_strategies(generate_strategy_grid()[0]))
    k, lo, hi = 4, 0, 2000
    with Engine(0) as probe:
        base = _held(probe)  # (a fresh engine's own tables; whatever other engines of the process hold)
        with Engine(0) as roomy:
            want = roomy.tournament(table, k, 7, lo, hi, shuffles_per_batch=500)["tally"]
            assert roomy.get_option("oom_replays") == 0
            held_roomy = _held(probe) - base
        hog = Engine(0)
        try:
            hog.hold_memory(300 << 20)
            base_tight = _held(probe)  # (+ the holder's own tables; the memory it holds on purpose is not counted)
            with Engine(0) as tight:
                tight.set_option("workspace_percent", 2000)
                got = tight.tournament(table, k, 7, lo, hi, shuffles_per_batch=500)["tally"]
                replays, budget = tight.get_option("oom_replays"), tight.get_option("last_budget")
                held_tight = _held(probe) - base_tight
        finally:
            hog.hold_memory(-1)
            hog.close()
        assert _held(probe) == base  # (held memory is not counted, and all three engines are gone)
    assert np.array_equal(got, want)
    assert replays >= 1 and budget < (6 << 30), (replays, budget)
    assert held_tight <= held_roomy, (held_tight, held_roomy)
