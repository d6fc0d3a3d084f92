"""The counter-overflow exit of the game kernels, taken to its end on the device, and games whose fields hold the last value they can.

tests/counter_limit_cases.py finds the games on the CPU oracle and tests/test_counter_limits_cpu.py asserts their premises; every comparison
here is bit-exact against the oracle (``pyoracle`` rows and tallies, ``oracle_engine_stub`` seat statistics, ``round_robin_engine_stub``).

a. Every compiled game-kernel instance (the 63 routes of ``kernel_instances.MATRIX``) plays a call in which one known game sits one
   round inside the 64 000-rolls band (``R_in``: equal to the oracle) and one round beyond it (``R_out``: ``FK_ERR_COUNTER_OVERFLOW``
   naming that game), then ``R_in`` again.  On a hot / cold route the long game reaches the cold record's farkle bit first, so what
   is compared there is the replay on ``fk_play_kernel``; the route's own instance is pinned by the same call without the long game.
b. Both host checks of a tournament call (per chunk, and deferred behind the last chunk's post-passes), with rows, column images and
   neither, with and without the chunk pipeline and with a hinted next range: after each failure the plain call and the lag call
   return what they returned before it, and the resident tally accumulator holds the successful calls only.
c. The cold record's farkle bit crossed by one (255 farkles: the hot / cold instance; 256: replayed).  Farkles are the only field of
   the seven that any game of the search space takes to its bit first (``counter_limit_cases.HOT_COLD_SEARCH``); the 63 000 returned-dice
   bands and the 65 500-point turn band of the play kernels cannot be reached before the rolls band either and stay host-checked
   (tests/native/roll_guards_host_check.hip).
d. Banked totals at the largest targets the record layouts hold (3 200 000 lean, 135 000 hot / cold, 3 200 050 full), actually reached.
e. The trace and census kernels' 65 535 limit: at ``R_in`` the trace's rows are the oracle's and its event counts the rows' rolls
   (tests/trace_oracle.py replays a seat's stream from its start for every roll: 65 000 rolls are out of its reach), the census equals
   the census of the trace's events and its per-strategy totals the oracle rows' sums; one round later the error names the smallest
   offending game, in a later census chunk by its index in the call.
f. The round robin returns the error and leaves the caller's summary untouched.

What a caller may assume after the error is what include/farkle_hip.h states and (b), (f) test: output buffers of the failed call are
unspecified, buffers a call adds to (resident tally, round-robin summary) are untouched, and the context is as before the call.

Seconds per case on an MI355X (the offender is one lane playing up to 64 000 x k rolls, five times per case of (a)):
  (a) hc_ns12_k11 2.3 - 2.6, hc_ns10_k10 2.1 - 2.2, hc_k8 1.8 - 1.9, hc_k7 1.6, every other route less (two seats: about 0.4); the
      eleven-seat routes therefore keep their ``R_in`` calls
  (b) under 0.8 each    (c), (d), (f) 0.1 or less each    (e) trace and census lists 2.2, tournament census 0.5    the file: about 80
"""
from __future__ import annotations

import re
from functools import lru_cache

import numpy as np
import pytest

import counter_limit_cases as clc
import kernel_instances as ki
from farkle_ii_amd.backend import FK_ERR_COUNTER_OVERFLOW, FarkleHipError, make_overrides

pytestmark = pytest.mark.gpu

_REACHED: dict[str, str] = {}  # instance -> route, for every route that launched its instance and left through the exit
ROUTE = {route.name: (inst, route) for inst, route in ki.MATRIX.items()}
C = clc.CALL


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


class _options:
    """``set_option`` for the block, ``OPTION_DEFAULTS`` (and whatever else was named) restored after it."""

    def __init__(self, eng, options, restore=()):
        self.eng, self.options, self.restore = eng, tuple(options), dict(restore)

    def __enter__(self):
        for name, value in self.options:
            self.eng.set_option(name, value)

    def __exit__(self, *exc):
        for name, value in {**ki.OPTION_DEFAULTS, **self.restore}.items():
            self.eng.set_option(name, value)


def _overflow_game(err) -> int:
    """The game a ``FK_ERR_COUNTER_OVERFLOW`` names."""
    assert err.value.code == FK_ERR_COUNTER_OVERFLOW, str(err.value)
    named = re.findall(r"game (\d+)\)", str(err.value))
    assert len(named) == 1, str(err.value)
    return int(named[0])


def _form_of(instance: str) -> str:
    return ki.instance_form(instance)


# ---- a. every instance leaves through the exit ----------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _call_oracle(form: str, k: int, S: int, rounds):
    from oracle_engine_stub import seat_stats_from_rows

    ref = clc.call_reference(clc.never_bank_table(form, S), k, rounds, offender=clc.play_case(form, k, S)["offender"], n_threads=8)
    ref["seat_stats"] = seat_stats_from_rows(ref["rows"], k, S, S // k, C["spb"])
    return ref


def _call(eng, table, k, offender, rounds, **kw):
    ov = make_overrides([clc.game_override(clc.ROOT, *offender, k, rounds)] if rounds is not None else [])
    return eng.tournament(table, k, clc.ROOT, C["begin"], C["end"], shuffles_per_batch=C["spb"], max_rounds=C["max_rounds"], overrides=ov, **kw)


def _equal(got, ref, what) -> None:
    assert np.array_equal(got["tally"], ref["tally"]), (what, np.argwhere(got["tally"] != ref["tally"])[:4])
    assert got["rows"].tobytes() == ref["rows"].tobytes(), what
    assert np.array_equal(got["seat_stats"], ref["seat_stats"]), (what, np.argwhere(got["seat_stats"] != ref["seat_stats"])[:4])


def _exit_of_a_tournament_route(eng, inst: str, route: ki.Route) -> None:
    case = clc.play_case(route.form, route.k, route.S)
    table, k = case["table"], route.k
    hot_cold = inst.startswith("fk_play_hc_kernel<")
    full = dict(want_rows=True, want_seat_stats=True, want_seat_ratios=False)
    _equal(_call(eng, table, k, case["offender"], None, **full), _call_oracle(route.form, k, route.S, None), (route.name, "no long game"))
    assert eng.last_play_instance() == inst, route.name  # the instance this route's calls launch
    for attempt in ("first", "again"):
        _equal(_call(eng, table, k, case["offender"], case["R_in"], **full), _call_oracle(route.form, k, route.S, case["R_in"]), (route.name, "R_in", attempt))
        ran = eng.last_play_instance()
        if hot_cold:  # 256 farkles come long before 64 000 rolls: the call was handed back and replayed
            assert ran.startswith("fk_play_kernel<") and _form_of(ran) == route.form, (route.name, ran)
        else:
            assert ran == inst, (route.name, ran)
        if attempt == "first":
            for wanted in (full, {}):  # with rows every chunk is checked as it ends; counts only: the check travels with the tally
                with pytest.raises(FarkleHipError) as err:
                    _call(eng, table, k, case["offender"], case["R_out"], **wanted)
                assert _overflow_game(err) == case["game"], (route.name, sorted(wanted), str(err.value))


def _h2h(eng, case, rounds, chunk_games=None):
    n = len(case["seats"])
    ov = make_overrides([case["override"](rounds)] if rounds is not None else [])
    return eng.h2h_blocks(case["seats"], clc.ROOT, case["pair"], case["order"], np.full(n, clc.H2H_ATTEMPTS), np.full(n, clc.H2H_ATTEMPTS),
                          chunk_games=chunk_games, max_rounds=C["max_rounds"], overrides=ov)


def _exit_of_the_h2h_route(eng, po, inst: str, route: ki.Route) -> None:
    case = clc.h2h_case(route.form, route.S)
    n = len(case["seats"])
    want = np.stack([po.h2h_block(case["seats"][b].view(po.STRATEGY_DTYPE), clc.ROOT, int(case["pair"][b]), int(case["order"][b]),
                                  clc.H2H_ATTEMPTS, clc.H2H_ATTEMPTS, clc.H2H_ATTEMPTS, max_rounds=C["max_rounds"],
                                  overrides=po.make_overrides([case["override"](case["R_in"])])) for b in range(n)])
    assert np.array_equal(want[:, :3], np.tile(np.array([3, 0, 3], dtype=np.uint64), (n, 1)))  # nobody banks: every attempt ends at its limit
    for attempt in ("first", "again"):
        assert np.array_equal(_h2h(eng, case, case["R_in"]), want), (route.name, attempt)
        assert eng.last_play_instance() == inst, route.name
        if attempt == "first":
            with pytest.raises(FarkleHipError) as err:  # an override list: the pass is finished by the per-launch check
                _h2h(eng, case, case["R_out"])
            assert _overflow_game(err) == case["game"], str(err.value)
    # without overrides the passes are pipelined and the error record travels through the pinned mailbox: one block, one attempt
    b = clc.H2H_OFFENDER[0]
    beyond = 17_000
    row = clc.h2h_game_row(case["seats"][b], clc.ROOT, int(case["pair"][b]), int(case["order"][b]), 0, beyond)
    assert row is None or clc.field_max(row, "rolls") > clc.PLAY_ROLLS_LIMIT
    with pytest.raises(FarkleHipError) as err:
        eng.h2h_blocks(case["seats"][b:b + 1], clc.ROOT, case["pair"][b:b + 1], case["order"][b:b + 1], 1, 1, max_rounds=beyond)
    assert _overflow_game(err) == 0
    assert np.array_equal(_h2h(eng, case, case["R_in"]), want), (route.name, "after the pipelined pass")


@pytest.mark.parametrize("inst", sorted(ki.MATRIX), ids=lambda inst: ki.MATRIX[inst].name)
def test_every_instance_leaves_through_the_overflow_exit(eng, po, inst):
    route = ki.MATRIX[inst]
    with _options(eng, route.options):
        if route.entry == "h2h_blocks":
            _exit_of_the_h2h_route(eng, po, inst, route)
        else:
            _exit_of_a_tournament_route(eng, inst, route)
    _REACHED[inst] = route.name


def test_the_exit_was_taken_on_every_compiled_instance():
    """Runs after the tests above."""
    from farkle_ii_amd import backend

    compiled = ki.compiled_instances(backend.library_path())
    assert set(_REACHED) == compiled, {"not reached": sorted(compiled - set(_REACHED)), "not compiled": sorted(set(_REACHED) - compiled)}
    assert len(compiled) == 63


# ---- b. both host checks, and the state left behind -----------------------------------------------------------------------------------

LAGS = (1, 2, 7)
IDS = ((np.arange(64, dtype=np.int64) * 37 + 11) % 257).astype(np.int32)
K = clc.CHUNKED
RANGE = (K["root"], K["begin"], K["end"])
PLAIN = dict(shuffles_per_batch=K["spb"], max_rounds=K["max_rounds"])
SMALL_CHUNKS = (("chunk_bytes", 1 << 20),)
RESTORE = {"chunk_bytes": 48 << 30, "pipeline": 1, "resident_tally": 0}


def _bytes_equal(got: dict, want: dict, what) -> None:
    assert got.keys() == want.keys(), what
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[key].dtype == w.dtype and got[key].shape == w.shape and got[key].tobytes() == w.tobytes(), (what, key)
        else:
            assert got[key] == w, (what, key)


@lru_cache(maxsize=None)
def _chunked_oracle(k: int):
    import pyoracle

    table = clc.never_bank_table("all", K["S"])
    return pyoracle.tournament(table.view(pyoracle.STRATEGY_DTYPE), k, *RANGE, shuffles_per_batch=K["spb"], max_rounds=K["max_rounds"], n_threads=8)


def _before(eng, table, k):
    plain = eng.tournament(table, k, *RANGE, **PLAIN)
    assert eng.timing()["play_launches"] >= 2  # a chunk that is checked as it ends, and a last one whose check is deferred
    assert np.array_equal(plain["tally"], _chunked_oracle(k)["tally"])
    return plain, eng.tournament_lags(table, k, *RANGE, LAGS, **PLAIN)


def _clean(eng, table, k, before, what) -> None:
    _bytes_equal(eng.tournament(table, k, *RANGE, **PLAIN), before[0], (what, "plain call after it"))
    _bytes_equal(eng.tournament_lags(table, k, *RANGE, LAGS, **PLAIN), before[1], (what, "lags call after it"))


FAILING = {
    "plain": lambda e, t, k, ov: e.tournament(t, k, *RANGE, overrides=ov, **PLAIN),                    # the last chunk's check is deferred
    "rows": lambda e, t, k, ov: e.tournament(t, k, *RANGE, overrides=ov, want_rows=True, **PLAIN),     # every chunk is checked as it ends
    "columns": lambda e, t, k, ov: e.tournament_columns(t, k, *RANGE, IDS, overrides=ov, **PLAIN),
}


def _fails_naming(eng, entry: str, case: dict) -> None:
    ov = make_overrides([clc.game_override(K["root"], *case["offender"], case["k"], case["R_out"])])
    with pytest.raises(FarkleHipError) as err:
        FAILING[entry](eng, case["table"], case["k"], ov)
    assert _overflow_game(err) == case["game"], (entry, str(err.value))


@pytest.mark.parametrize("pipeline", [1, 0])
@pytest.mark.parametrize("k", [2, 4])
def test_a_failed_chunked_call_leaves_the_context_as_it_was(eng, k, pipeline):
    table = clc.never_bank_table("all", K["S"])
    with _options(eng, SMALL_CHUNKS + (("pipeline", pipeline),), RESTORE):
        before = _before(eng, table, k)
        for where in ("first", "last"):
            for entry in FAILING:
                _fails_naming(eng, entry, clc.chunked_case(k, where))
                _clean(eng, table, k, before, (k, pipeline, where, entry))


@pytest.mark.parametrize("k", [2, 4])
def test_a_failed_call_with_a_hinted_next_range_and_a_resident_tally(eng, k):
    table = clc.never_bank_table("all", K["S"])
    case = clc.chunked_case(k, "last")  # the hinted range is prepared beside the last chunk's game kernel: the one that raises
    nxt = (K["root"], K["end"], K["end"] + 100)
    with _options(eng, SMALL_CHUNKS, RESTORE):
        before = _before(eng, table, k)
        hinted_before = eng.tournament(table, k, *nxt, **PLAIN)
        eng.hint_next(nxt[1], nxt[2])
        _fails_naming(eng, "plain", case)
        _bytes_equal(eng.tournament(table, k, *nxt, **PLAIN), hinted_before, "the hinted range after the failed call")
        _clean(eng, table, k, before, (k, "hinted"))
        # resident tally: a failed call adds nothing, whichever check finds the error
        eng.set_option("resident_tally", 1)
        total = eng.tournament(table, k, *RANGE, **PLAIN)["tally"].copy()
        for entry, where in (("plain", "last"), ("plain", "first"), ("rows", "last")):
            _fails_naming(eng, entry, clc.chunked_case(k, where))
        total += eng.tournament(table, k, *RANGE, **PLAIN)["tally"]
        assert np.array_equal(eng.reduce_resident_tally(total.shape), total)
        assert total.any()


# ---- c. the cold record's farkle bit, crossed by one ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k,name", [(4, "hc_cold_in_lds_k4"), (8, "hc_k8")])
def test_hot_cold_farkle_bit_is_crossed_by_one(eng, k, name):
    from oracle_engine_stub import seat_stats_from_rows

    assert list(clc.hot_cold_cases()) == ["farkles"]
    last = clc.hot_cold_cases()["farkles"]["R"]
    assert last == clc.HC_GUARDS["farkles"] - 1
    for form in ki.FORMS:
        inst, route = ROUTE[f"{name}-{form}"]
        table = clc.never_bank_table(form, route.S)
        with _options(eng, route.options):
            for rounds in (last, last + 1):  # every seat of every game holds `rounds` farkles
                ref = clc.call_reference(table, k, None, call={**C, "max_rounds": rounds}, n_threads=8)
                assert (ref["rows"]["seats"]["farkles"] == rounds).all()
                ref["seat_stats"] = seat_stats_from_rows(ref["rows"], k, route.S, route.S // k, C["spb"])
                got = eng.tournament(table, k, clc.ROOT, C["begin"], C["end"], shuffles_per_batch=C["spb"], max_rounds=rounds, want_rows=True,
                                     want_seat_stats=True, want_seat_ratios=False)
                ran = eng.last_play_instance()
                if rounds == last:
                    assert ran == inst, (form, ran)
                else:
                    assert ran.startswith("fk_play_kernel<") and _form_of(ran) == form, (form, ran)
                _equal(got, ref, (name, form, rounds))


# ---- d. fields at their real maxima ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,target", [("lean768_k2", clc.LEAN_TARGET), ("lean768_k3", clc.LEAN_TARGET), ("full256_k4", clc.FULL_TARGET),
                                         ("hc_cold_in_lds_k4", clc.HC_TARGET), ("hc_k6", clc.HC_TARGET), ("hc_k8", clc.HC_TARGET)])
def test_banked_totals_reach_the_largest_targets(eng, name, target):
    from oracle_engine_stub import seat_stats_from_rows

    inst, route = ROUTE[f"{name}-none"]
    table, ref = clc.maxima_reference(route.k, route.S, target)
    assert (clc.winners_scores(ref["rows"]) >= target).all()  # the targets are reached, not merely planned for
    with _options(eng, route.options):
        got = eng.tournament(table, route.k, clc.ROOT, 0, 1, target_score=target, max_rounds=clc.MAXIMA_ROUNDS, want_rows=True,
                             want_seat_stats=True, want_seat_ratios=False)
        assert eng.last_play_instance() == inst
        want = dict(ref, seat_stats=seat_stats_from_rows(ref["rows"], route.k, route.S, route.S // route.k, 1))
        _equal(got, want, (name, target))
        counts = eng.tournament(table, route.k, clc.ROOT, 0, 1, target_score=target, max_rounds=clc.MAXIMA_ROUNDS)
        assert eng.last_play_instance() == inst and np.array_equal(counts["tally"], ref["tally"])


def test_batched_h2h_block_reaches_the_largest_lean_target(eng, po):
    inst, route = ROUTE["h2h_blocks-none"]
    seats = clc.bank_at_once_table(2)
    want = po.h2h_block(seats.view(po.STRATEGY_DTYPE), clc.ROOT, 9, 1, 3, 6, 6, target_score=clc.LEAN_TARGET, max_rounds=clc.MAXIMA_ROUNDS)
    assert want.tolist()[:3] == [3, 3, 0]  # three attempts, each played to 3 200 000 points
    got = eng.h2h_blocks(seats, clc.ROOT, [9], [1], 3, 6, target_score=clc.LEAN_TARGET, max_rounds=clc.MAXIMA_ROUNDS)
    assert eng.last_play_instance() == inst
    assert np.array_equal(got[0], want)


# ---- e. trace and census --------------------------------------------------------------------------------------------------------------

def test_trace_and_census_at_and_beyond_65535_rolls(eng):
    from farkle_ii_amd.roll_census import RollCensus
    from test_roll_census_gpu import assert_same

    case = clc.trace_case()
    coords, table, ss = case["coords"], case["table"], case["ss"]
    args = dict(target_score=clc.TRACE_TARGET, max_rounds=case["R_in"])
    want_rows = case["rows"]([0, 1, 2], case["R_in"])
    rows, begin, events = eng.trace_games(coords, table, ss, 2, **args)
    assert rows.tobytes() == want_rows.tobytes()
    rolls = want_rows["seats"]["rolls"].astype(np.int64)
    assert rolls[1].max() == rolls[2].max() == clc.U16_LIMIT  # the last value the fields hold
    assert np.array_equal(np.diff(begin), rolls.sum(axis=1)) and len(events) == int(begin[-1])
    for g in range(3):  # per seat: as many events as the oracle's row counts rolls, as many farkles as it counts
        ev = events[begin[g]:begin[g + 1]]
        assert np.array_equal(np.bincount(ev["seat"], minlength=2), rolls[g])
        assert np.array_equal(np.bincount(ev["seat"][ev["points"] == 0], minlength=2), want_rows["seats"]["farkles"][g])
    census = RollCensus.from_engine(eng.census_games(coords, table, ss, 2, **args))
    assert_same(census, RollCensus.from_events(events, begin, ss, len(table), 256))
    per_strategy = np.zeros((len(table), 3), dtype=np.int64)
    for name, col in (("rolls", 0), ("farkles", 1), ("n_turns", 2)):
        np.add.at(per_strategy[:, col], ss.reshape(-1), want_rows["seats"][name].astype(np.int64).reshape(-1))
    assert np.array_equal(census.strategy_dice[:, :, 0].sum(axis=1), per_strategy[:, 0])
    assert np.array_equal(census.strategy_dice[:, :, 1].sum(axis=1), per_strategy[:, 1])
    assert np.array_equal(census.strategy_turns[:, 0], per_strategy[:, 2]) and np.array_equal(census.strategy_turns[:, 1], per_strategy[:, 1])
    # one round later both never-banking games are beyond 16 bits: the smaller index is named
    for call in (eng.trace_games, eng.census_games):
        with pytest.raises(FarkleHipError) as err:
            call(coords, table, ss, 2, target_score=clc.TRACE_TARGET, max_rounds=case["R_both"])
        assert _overflow_game(err) == 1, (call.__name__, str(err.value))
        with pytest.raises(FarkleHipError) as err:  # without game 1 it is game 2, now at index 1 ...
            call(coords[[0, 2]], table, ss[[0, 2]], 2, target_score=clc.TRACE_TARGET, max_rounds=case["R_both"])
        assert _overflow_game(err) == 1, (call.__name__, str(err.value))
        with pytest.raises(FarkleHipError) as err:  # ... and in front of the game that ends at its target, at index 0
            call(coords[[2, 0]], table, ss[[2, 0]], 2, target_score=clc.TRACE_TARGET, max_rounds=case["R_both"])
        assert _overflow_game(err) == 0, (call.__name__, str(err.value))
    assert eng.trace_games(coords, table, ss, 2, **args)[0].tobytes() == want_rows.tobytes()  # the same context afterwards


def test_tournament_census_names_the_game_of_a_later_chunk(eng):
    from farkle_ii_amd.roll_census import RollCensus

    case, cc = clc.census_case(), clc.CENSUS_CALL
    table, k = case["table"], cc["k"]

    def run(rounds):
        ov = make_overrides([clc.game_override(clc.ROOT, *cc["offender"], k, rounds)])
        return eng.tournament_census(table, k, clc.ROOT, cc["begin"], cc["end"], max_rounds=cc["max_rounds"], overrides=ov)

    eng.set_option("census_chunk_games", cc["chunk_games"])
    try:
        got = RollCensus.from_engine(run(case["R_in"]))
        assert eng.timing()["play_launches"] == 2
        with pytest.raises(FarkleHipError) as err:
            run(case["R_out"])
        assert _overflow_game(err) == case["game"]
    finally:
        eng.set_option("census_chunk_games", 0)
    rows = clc.call_reference(table, k, case["R_in"], call={"begin": cc["begin"], "end": cc["end"], "spb": 8, "max_rounds": cc["max_rounds"]},
                              offender=cc["offender"])["rows"]
    per_strategy = np.zeros((len(table), 3), dtype=np.int64)
    for name, col in (("rolls", 0), ("farkles", 1), ("n_turns", 2)):
        np.add.at(per_strategy[:, col], rows["seats"]["strategy"].reshape(-1), rows["seats"][name].astype(np.int64).reshape(-1))
    assert np.array_equal(got.strategy_dice[:, :, 0].sum(axis=1), per_strategy[:, 0])
    assert np.array_equal(got.strategy_turns[:, 0], per_strategy[:, 2]) and np.array_equal(got.strategy_turns[:, 1], per_strategy[:, 1])
    assert RollCensus.from_engine(run(case["R_in"])).equals(got)  # in one chunk


# ---- f. round robin -------------------------------------------------------------------------------------------------------------------

def test_round_robin_returns_the_error_and_leaves_the_summary_untouched(eng):
    import round_robin_engine_stub as rr

    table = rr.hard_table()[:4]  # rows 0 and 1 never bank: their pair's games run into the rolls band
    summary = np.arange(32, dtype=np.int64).reshape(4, 8) * 3 + 1
    keep = summary.copy()
    with pytest.raises(FarkleHipError) as err:
        eng.h2h_round_robin(table, clc.ROOT, 1, 1, max_rounds=17_000, summary=summary)
    _overflow_game(err)
    assert np.array_equal(summary, keep)
    good = dict(root_seed=clc.ROOT, target=5, max_attempts=10, max_rounds=24)
    want_states, want_summary = rr.Engine().h2h_round_robin(table, summary=keep.copy(), **good)
    states, out = eng.h2h_round_robin(table, summary=summary, **good)
    assert out is summary and np.array_equal(states, want_states) and np.array_equal(summary, want_summary)
