"""Every game-kernel instance of the library, in every strategy-flag form, against the CPU oracle (bit-exact).

For each route of tests/kernel_instances.py (MATRIX: one per compiled template instance) and each flag table of the route's form, the options
are set, the table is played, the library must report exactly that instance (``last_play_instance``), and per-batch tallies, rows,
permutations, all-seat statistics and the float64 ratio sums must equal the oracle's — at a full target with one batch (the LDS tally of the
LDS-record kernel) and at a short target with round limits, per-game overrides and several batches (result records, safety-limit and
final-round games).  The batched head-to-head instance plays blocks drawn from the same tables against the oracle's serial block loop.  The
last test checks that the routes reached every instance the library holds.

The tables of the two narrow forms share flags as 0 as well as 1 (kernel_instances.flag_tables): in those instances the shared flags come
from the launch argument ``PlayArgs.uflags``, not from the strategy."""
from __future__ import annotations

import zlib
from functools import lru_cache

import numpy as np
import pytest

import kernel_instances as ki

pytestmark = pytest.mark.gpu

_REACHED: dict[str, str] = {}  # instance -> route, for every route that reported its instance and matched the oracle


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle

    return pyoracle


# (root seed, first shuffle, shuffles, shuffles per batch, target, max_rounds, with overrides)
PARAMS = {"full": (17, 3, 8, 8, 10_000, 200, False), "short": (23, 0, 12, 4, 1_500, 4, True)}


def _overrides(root: int, k: int, gps: int):
    # (root, shuffle, game, k, max_rounds): a game with no round, one cut short, others allowed past the call's limit
    return [(root, 1, 0, k, 0), (root, 2, gps - 1, k, 1), (root, 5, 3 % gps, k, 9), (root, 9, 1, k, 30), (root, 10, gps // 2, k, 2)]


@lru_cache(maxsize=None)
def _tables(form: str, S: int):
    return ki.flag_tables(form, S)


@lru_cache(maxsize=None)
def _oracle(form: str, S: int, table_name: str, k: int, param: str):
    import pyoracle as po
    from oracle_engine_stub import seat_ratio_sums_from_rows, seat_stats_from_rows

    root, begin, n_sh, spb, target, mr, with_ov = PARAMS[param]
    table = _tables(form, S)[table_name]
    ov = po.make_overrides(_overrides(root, k, S // k)) if with_ov else None
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, root, begin, begin + n_sh, shuffles_per_batch=spb, target_score=target,
                        max_rounds=mr, overrides=ov, want_rows=True, want_perms=True, n_threads=8)
    ref["seat_stats"] = seat_stats_from_rows(ref["rows"], k, S, S // k, spb)
    ref["seat_ratio_sums"] = seat_ratio_sums_from_rows(ref["rows"], k, S, S // k, spb)
    return ref


def _check_tournament(eng, inst: str, route: ki.Route, table_name: str, table: np.ndarray, param: str) -> None:
    from farkle_ii_amd.backend import make_overrides

    k, S = route.k, route.S
    root, begin, n_sh, spb, target, mr, with_ov = PARAMS[param]
    ref = _oracle(route.form, S, table_name, k, param)
    ov = make_overrides(_overrides(root, k, S // k)) if with_ov else None
    what = (route.name, table_name, param)
    got = eng.tournament(table, k, root, begin, begin + n_sh, shuffles_per_batch=spb, target_score=target, max_rounds=mr, overrides=ov,
                         want_rows=True, want_perms=True, want_seat_stats=True)
    assert eng.last_play_instance() == inst, what
    assert np.array_equal(got["perms"], ref["perms"]), what
    assert np.array_equal(got["tally"], ref["tally"]), (what, np.argwhere(got["tally"] != ref["tally"])[:4])
    assert got["rows"].tobytes() == ref["rows"].tobytes(), what
    assert np.array_equal(got["seat_stats"], ref["seat_stats"]), (what, np.argwhere(got["seat_stats"] != ref["seat_stats"])[:4])
    assert got["seat_ratio_sums"].tobytes() == ref["seat_ratio_sums"].tobytes(), what
    # the same call for counts only: no state records wanted (one batch: the LDS tally wherever the instance keeps one)
    counts = eng.tournament(table, k, root, begin, begin + n_sh, shuffles_per_batch=spb, target_score=target, max_rounds=mr, overrides=ov)
    assert eng.last_play_instance() == inst, what
    assert np.array_equal(counts["tally"], ref["tally"]), what


def _check_h2h_blocks(eng, po, inst: str, route: ki.Route, table_name: str, table: np.ndarray, param: str) -> None:
    from farkle_ii_amd.backend import make_overrides

    root, _, _, _, target_score, mr, with_ov = PARAMS[param]
    rng = np.random.default_rng(zlib.crc32(f"{table_name}/{param}".encode()))
    seats = table[rng.permutation(len(table))].reshape(-1, 2)  # every strategy in one block: the blocks' table is the whole table
    n = len(seats)
    pair = rng.integers(0, 40, n).astype(np.uint64)
    order = rng.integers(0, 2, n).astype(np.uint32)
    target = rng.integers(1, 25, n).astype(np.uint64)
    max_attempts = (target * rng.choice([1, 2], n)).astype(np.uint64)
    ovs = [(root, int(pair[1]), 0, int(order[1]), 0), (root, int(pair[3]), 2, int(order[3]), 9), (root, int(pair[4]), 1, int(order[4]), 1)]
    ovs = ovs if with_ov else []
    chunk = 5 if with_ov else None  # short form: every block advanced five attempts per pass, then resumed to the end
    got = eng.h2h_blocks(seats, root, pair, order, target, max_attempts, chunk_games=chunk, target_score=target_score, max_rounds=mr,
                         overrides=make_overrides(ovs))
    assert eng.last_play_instance() == inst, (route.name, table_name, param)
    if chunk is not None:
        got = eng.h2h_blocks(seats, root, pair, order, target, max_attempts, chunk_games=10**9, target_score=target_score, max_rounds=mr,
                             overrides=make_overrides(ovs), states=got)
        assert eng.last_play_instance() == inst, (route.name, table_name, param)
    for b in range(n):  # (a block advanced in passes and resumed ends where one serial run of it ends)
        want = po.h2h_block(seats[b].view(po.STRATEGY_DTYPE), root, int(pair[b]), int(order[b]), int(target[b]), int(max_attempts[b]),
                            int(max_attempts[b]), target_score=target_score, max_rounds=mr, overrides=po.make_overrides(ovs))
        assert np.array_equal(got[b], want), (route.name, table_name, param, b, got[b], want)


@pytest.mark.parametrize("inst", sorted(ki.MATRIX), ids=lambda inst: ki.MATRIX[inst].name)
def test_instance_matches_oracle_on_every_flag_table_of_its_form(eng, po, inst):
    route = ki.MATRIX[inst]
    try:
        for name, value in route.options:
            eng.set_option(name, value)
        for table_name, table in _tables(route.form, route.S).items():
            for param in PARAMS:
                if route.entry == "h2h_blocks":
                    _check_h2h_blocks(eng, po, inst, route, table_name, table, param)
                else:
                    _check_tournament(eng, inst, route, table_name, table, param)
    finally:
        for name, value in ki.OPTION_DEFAULTS.items():
            eng.set_option(name, value)
    _REACHED[inst] = route.name


def test_the_routes_reached_every_compiled_instance():
    """Runs after the tests above: every instance the library holds was launched and equalled the oracle."""
    from farkle_ii_amd import backend

    compiled = ki.compiled_instances(backend.library_path())
    assert set(_REACHED) == compiled, {"not reached": sorted(compiled - set(_REACHED)), "not compiled": sorted(set(_REACHED) - compiled)}
    assert len(compiled) == 63
