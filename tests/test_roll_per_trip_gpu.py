"""The two-seat roll loop without its per-trip guard compares, flag write-back and increment load (round 12), bit-compared with the CPU
oracle.  The two-seat lean instances (``fk_play_kernel<768, true, 6, MIXED, false, BLK, 2>``) test the three u16 counter bands every
``RG_SAMPLE_TRIPS`` = 32 trips of a wave and where a game ends (csrc/fk_device.h: ``sampled_overflow50``, ``game_end_overflow50``),
write ``has_buf`` back as a toggle, and carry both seats' PCG increments in registers (the owner's and the xor of the two).

a. Results: k = 2 with 64 and with 6 strategies; 64, 65 and 1 shuffles (a wave's worth of games per block row, one more, one); the flat
   and the general copy of the loop nest (option ``flat_handover`` 1 / 0); the three flag forms; rows and seat statistics, which read
   both records where a game ends; a game-list launch; and the forced-detour build, whose replayed rolls leave ``has_buf`` to the
   sequential path.
b. The counter-overflow exit, on every two-seat instance and both copies, built on tests/counter_limit_cases.py: the long game's busiest
   seat holds exactly 64 000 rolls after ``R_in`` rounds.
     - ``R_in``: one round inside, no error, equal to the oracle;
     - ``R_in + 1``: the field crosses the band in the game's last round, fewer than 32 trips before the game ends — unless one of the
       wave's sample points happens to fall into those trips, only the game-end test sees it;
     - ``R_in + 100``: the game crosses and plays on for some 800 trips: a sample point raises, long before the game's end;
     - the busiest seat is seat 0 in one long game and seat 1 in another: seat 1's record is the one the end of a game otherwise reads
       the score word of and nothing else (nobody banks: seat 0 "wins" the tie).
   Each error names the long game, and the call after it returns the oracle's result again.

Seconds on an MI355X: (a) under 0.2 each; (b) about 0.4 per call of a long game, 2 to 3 per case."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import counter_limit_cases as clc
import kernel_instances as ki
from farkle_ii_amd.backend import FK_ERR_COUNTER_OVERFLOW, FarkleHipError, make_overrides

pytestmark = pytest.mark.gpu

ROUTE = {route.name: (inst, route) for inst, route in ki.MATRIX.items()}
C = clc.CALL
PLAYS_ON = 100  # rounds beyond R_in: about 400 more rolls of either seat, a dozen sample points


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.set_option("flat_handover", 1)
    e.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle

    return pyoracle


@lru_cache(maxsize=None)
def _grid(S: int) -> np.ndarray:
    """The benchmark's 64-strategy grid (require_both and favor_score vary), or its first S rows with the other flags varied too."""
    from farkle_ii_amd.strategies import generate_strategy_grid, pack_strategies

    strategies, _ = generate_strategy_grid(
        score_thresholds=[250, 300, 350, 400], dice_thresholds=[0, 1, 2, 3], smart_five_opts=[True], smart_one_opts=[True],
        consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[True])
    table = pack_strategies(strategies)
    assert len(table) == 64
    return table


def _table(form: str, S: int) -> np.ndarray:
    t = _grid(64)[np.linspace(0, 63, S).astype(int)].copy()
    i = np.arange(S)
    t["require_both"], t["favor_score"] = (0, 0) if form == "none" else (i & 1, (i >> 1) & 1)
    if form == "all":
        t["smart_one"], t["auto_hot_dice"], t["run_up_score"] = i & 1, (i >> 1) & 1, (i // 3) & 1
    t["strategy_id"] = i
    ki.check_legal(t)
    assert ki.table_form(t) == form
    return t


@lru_cache(maxsize=None)
def _ref(form: str, S: int, shuffles: int):
    import pyoracle as po

    return po.tournament(_table(form, S).view(po.STRATEGY_DTYPE), 2, 42, 0, shuffles, want_rows=True, n_threads=8)


# ---- a. results ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flat", [1, 0], ids=["flat", "general"])
@pytest.mark.parametrize("form", list(ki.FORMS))
@pytest.mark.parametrize("S,shuffles", [(64, 64), (64, 65), (64, 1), (6, 64), (6, 65), (6, 1)])
def test_two_seat_results_equal_the_oracle(eng, po, S, shuffles, form, flat):
    from oracle_engine_stub import seat_stats_from_rows

    table, ref = _table(form, S), _ref(form, S, shuffles)
    eng.set_option("flat_handover", flat)
    try:
        counts = eng.tournament(table, 2, 42, 0, shuffles)  # tallies in LDS
        assert eng.last_play_instance() == f"fk_play_kernel<768, true, 6, {ki.FORMS[form]}u, false, false, 2>"
        got = eng.tournament(table, 2, 42, 0, shuffles, want_rows=True, want_seat_stats=True)
    finally:
        eng.set_option("flat_handover", 1)
    assert np.array_equal(counts["tally"][0], ref["tally"].sum(axis=0))
    assert np.array_equal(got["tally"], ref["tally"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()
    assert np.array_equal(got["seat_stats"], seat_stats_from_rows(ref["rows"], 2, S, S // 2, shuffles))


def test_game_list_launch(eng, po):
    from farkle_ii_amd.backend import COORD_DTYPE

    table = _table("all", 64)
    coords = np.zeros(200, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 10, 123, 2, np.arange(200)
    seat = np.stack([(np.arange(200) * 7) % 64, (np.arange(200) * 11 + 3) % 64], axis=1).astype(np.int32)
    rows = eng.play_games(coords, table, seat, 2)
    assert eng.last_play_instance().endswith("false, 2>")
    assert rows.tobytes() == po.play_games(coords.view(po.COORD_DTYPE), table.view(po.STRATEGY_DTYPE), seat, 2).tobytes()


def test_h2h_block_instance(eng, po):
    seats = _grid(64)[[3, 40]]
    got = eng.h2h(seats, 42, 5, 0, 2000, 4000, 10**6)
    assert eng.last_play_instance().endswith("true, 2>")  # BLK, two seats
    assert np.array_equal(got, po.h2h_block(seats.view(po.STRATEGY_DTYPE), 42, 5, 0, 2000, 4000, 10**6))


def test_forced_detours(po):
    """libfarkle_hip_detour.so: every fourth roll is replayed sequentially and hands its own ``has_buf`` to the toggle."""
    from farkle_ii_amd import backend

    backend.build_library(variant="detour")  # prebuilt by __graft_entry__.build()
    detour = backend.Engine(0, variant="detour")
    try:
        for form in ki.FORMS:
            ref = _ref(form, 64, 65)
            got = detour.tournament(_table(form, 64), 2, 42, 0, 65, want_rows=True)
            assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes(), form
    finally:
        detour.close()


# ---- b. the counter-overflow exit ----------------------------------------------------------------------------------------------------

def _names(err, game: int, what) -> None:
    import re

    assert err.value.code == FK_ERR_COUNTER_OVERFLOW, (what, str(err.value))
    assert [int(g) for g in re.findall(r"game (\d+)\)", str(err.value))] == [game], (what, str(err.value))


# (form, busiest seat) -> the first game of the offender's shuffle (S = 96) whose busiest seat is that one and holds exactly 64 000 rolls
# after R_in rounds while the other seat holds fewer (found with ``clc.boundary`` over the games of the shuffle; asserted below)
LONG_GAMES = {("none", 0): 12, ("none", 1): 18, ("rb_fav", 0): 12, ("rb_fav", 1): 18, ("all", 0): 44, ("all", 1): 0}


@lru_cache(maxsize=None)
def _long_game(form: str, S: int, busiest: int) -> dict:
    g = LONG_GAMES[(form, busiest)]
    b = clc.boundary(clc.never_bank_table(form, S), 2, clc.ROOT, clc.OFFENDER_SHUFFLE, g, "rolls", clc.PLAY_ROLLS_LIMIT, guess=15_000)
    return {"offender": (clc.OFFENDER_SHUFFLE, g), "game": (clc.OFFENDER_SHUFFLE - C["begin"]) * (S // 2) + g, **b}


@lru_cache(maxsize=None)
def _call_ref(form: str, S: int, offender: tuple, rounds: int):
    return clc.call_reference(clc.never_bank_table(form, S), 2, rounds, offender=offender, n_threads=8)


def _call(eng, table, offender, rounds, **kw):
    ov = make_overrides([clc.game_override(clc.ROOT, *offender, 2, rounds)])
    return eng.tournament(table, 2, clc.ROOT, C["begin"], C["end"], shuffles_per_batch=C["spb"], max_rounds=C["max_rounds"], overrides=ov, **kw)


@pytest.mark.parametrize("flat", [1, 0], ids=["flat", "general"])
@pytest.mark.parametrize("busiest", [0, 1], ids=["seat0", "seat1"])
@pytest.mark.parametrize("form", list(ki.FORMS))
def test_tournament_instances_report_a_band_at_a_sample_point_and_at_the_games_end(eng, form, busiest, flat):
    inst, route = ROUTE[f"lean768_k2-{form}"]
    assert route.S == 96
    case = _long_game(form, route.S, busiest)
    table = clc.never_bank_table(form, route.S)
    assert int(case["row_in"]["seats"]["rolls"][busiest]) == clc.PLAY_ROLLS_LIMIT > int(case["row_in"]["seats"]["rolls"][busiest ^ 1])
    for name, value in route.options + (("flat_handover", flat),):
        eng.set_option(name, value)
    try:
        def inside(what):
            got, ref = _call(eng, table, case["offender"], case["R_in"], want_rows=True), _call_ref(form, route.S, case["offender"], case["R_in"])
            assert eng.last_play_instance() == inst, what
            assert np.array_equal(got["tally"], ref["tally"]) and got["rows"].tobytes() == ref["rows"].tobytes(), what

        inside("one round inside")
        for beyond in (1, PLAYS_ON):  # caught where the game ends (or at a sample point of its last trips); caught at a sample point
            for wanted in ({"want_rows": True}, {}):
                with pytest.raises(FarkleHipError) as err:
                    _call(eng, table, case["offender"], case["R_in"] + beyond, **wanted)
                _names(err, case["game"], (form, busiest, flat, beyond, sorted(wanted)))
            inside(("the call after the error", beyond))
    finally:
        for name, value in {**ki.OPTION_DEFAULTS, "flat_handover": 1}.items():
            eng.set_option(name, value)


@pytest.mark.parametrize("form", list(ki.FORMS))
def test_h2h_block_instances_report_a_band_at_a_sample_point_and_at_the_games_end(eng, po, form):
    inst, route = ROUTE[f"h2h_blocks-{form}"]
    case = clc.h2h_case(form, route.S)
    n = len(case["seats"])

    def run(rounds):
        return eng.h2h_blocks(case["seats"], clc.ROOT, case["pair"], case["order"], np.full(n, clc.H2H_ATTEMPTS), np.full(n, clc.H2H_ATTEMPTS),
                              max_rounds=C["max_rounds"], overrides=make_overrides([case["override"](rounds)]))

    want = np.stack([po.h2h_block(case["seats"][b].view(po.STRATEGY_DTYPE), clc.ROOT, int(case["pair"][b]), int(case["order"][b]),
                                  clc.H2H_ATTEMPTS, clc.H2H_ATTEMPTS, clc.H2H_ATTEMPTS, max_rounds=C["max_rounds"],
                                  overrides=po.make_overrides([case["override"](case["R_in"])])) for b in range(n)])
    assert np.array_equal(run(case["R_in"]), want)
    assert eng.last_play_instance() == inst
    for beyond in (1, PLAYS_ON):
        with pytest.raises(FarkleHipError) as err:
            run(case["R_in"] + beyond)
        _names(err, case["game"], (form, beyond))
        assert np.array_equal(run(case["R_in"]), want), (form, "the call after the error", beyond)
