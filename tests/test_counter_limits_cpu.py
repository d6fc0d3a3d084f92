"""The premises of tests/test_counter_limits_gpu.py, asserted on the CPU oracle alone (tests/counter_limit_cases.py finds the cases).

Conditions, not measurements: in every call exactly one game leaves the limit at ``R_out`` and its counters still fit 16 bits, at ``R_in``
it sits within one round of the limit, no other game of the call comes within a factor of two of any guard, the tables are legal and of
the flag form their route asks for, and the committed result of the hot / cold search says what the oracle says."""
from __future__ import annotations

import numpy as np
import pytest

import counter_limit_cases as clc
import kernel_instances as ki

SHAPES = sorted({(r.form, r.k, r.S) for r in ki.MATRIX.values() if r.entry == "tournament"})


def _at_the_edge(case: dict, limit: int, exact: bool = False) -> None:
    """``row_in`` within one round's rolls of the limit, ``row_out`` beyond it in a field that still fits 16 bits."""
    rolls_in, rolls_out = (case[name]["seats"]["rolls"].astype(np.int64) for name in ("row_in", "row_out"))
    assert case["R_out"] == case["R_in"] + 1
    assert int(case["row_in"]["n_rounds"]) == case["R_in"] and int(case["row_out"]["n_rounds"]) == case["R_out"]
    assert rolls_in.max() <= limit < rolls_out.max() <= clc.U16_LIMIT
    assert not exact or rolls_in.max() == limit  # the last value the guard lets through
    one_round = int((rolls_out - rolls_in).max())
    assert 0 < one_round <= 1000 and limit - rolls_in.max() < one_round
    for name in ("n_smart_five_dice", "n_smart_one_dice"):  # the rolls band is the only one that is crossed
        assert int(case["row_out"]["seats"][name].max()) <= 63_000
    assert int(case["row_out"]["seats"]["highest_turn"].max()) <= 65_500


def _others_far_inside(rows, offender: int) -> None:
    others = np.delete(rows, offender)
    assert int(others["seats"]["rolls"].max()) * 2 < min(clc.PLAY_ROLLS_LIMIT, clc.HC_GUARDS["rolls"])
    for name, bit in clc.HC_GUARDS.items():
        assert int(others["seats"][name].max()) * 2 < bit, name
    assert int(others["seats"]["highest_turn"].max()) * 2 < 65_500


def test_the_tables_are_legal_and_of_their_form():
    for form in ki.FORMS:
        for S in (8, 24, 64, 96, 98, 99, 100):
            table = clc.never_bank_table(form, S)
            ki.check_legal(table)
            assert ki.table_form(table) == form and len(table) == S
            assert (table["consider_dice"] == 1).all() and (table["dice_threshold"] == -1).all()
    ki.check_legal(clc.bank_at_once_table(96))
    assert len(list(clc.legal_flag_forms())) == 120


@pytest.mark.parametrize("form,k,S", SHAPES, ids=lambda v: str(v))
def test_one_game_of_the_call_crosses_the_rolls_band(form, k, S):
    case = clc.play_case(form, k, S)
    _at_the_edge(case, clc.PLAY_ROLLS_LIMIT, exact=True)
    assert case["offender"][0] == clc.OFFENDER_SHUFFLE and clc.CALL["begin"] <= clc.OFFENDER_SHUFFLE < clc.CALL["end"]
    for rounds, name in ((case["R_in"], "row_in"), (case["R_out"], "row_out")):
        rows = clc.call_reference(case["table"], k, rounds, offender=case["offender"])["rows"]
        assert rows[case["game"]].tobytes() == case[name].tobytes()
        beyond = np.flatnonzero(rows["seats"]["rolls"].max(axis=1) > clc.PLAY_ROLLS_LIMIT)
        assert beyond.tolist() == ([case["game"]] if name == "row_out" else [])
        _others_far_inside(rows, case["game"])
        assert (rows["seats"]["score"] == 0).all() and (rows["seats"]["farkles"] == rows["seats"]["n_turns"]).all()  # nobody ever banks


@pytest.mark.parametrize("form", list(ki.FORMS))
def test_one_attempt_of_the_head_to_head_call_crosses_the_rolls_band(form):
    case = clc.h2h_case(form, 96)
    _at_the_edge(case, clc.PLAY_ROLLS_LIMIT, exact=True)
    assert ki.table_form(case["seats"].reshape(-1)) == form
    b, attempt = clc.H2H_OFFENDER
    assert case["game"] == b * clc.H2H_ATTEMPTS + attempt and len(set(case["pair"].tolist())) == len(case["pair"])
    for blk in range(len(case["seats"])):  # every other attempt stops at the call's six rounds
        for a in range(clc.H2H_ATTEMPTS):
            if (blk, a) != clc.H2H_OFFENDER:
                row = clc.h2h_game_row(case["seats"][blk], clc.ROOT, int(case["pair"][blk]), int(case["order"][blk]), a, clc.CALL["max_rounds"])
                assert int(row["status"]) == 1 and int(row["seats"]["rolls"].max()) * 2 < clc.HC_GUARDS["rolls"]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("where", ["first", "last"])
def test_the_chunked_calls_offender(k, where):
    case = clc.chunked_case(k, where)
    _at_the_edge(case, clc.PLAY_ROLLS_LIMIT)
    n_games = (clc.CHUNKED["end"] - clc.CHUNKED["begin"]) * (clc.CHUNKED["S"] // k)
    assert case["game"] == (1 if where == "first" else n_games - 1)
    assert ki.table_form(case["table"]) == "all"


@pytest.mark.parametrize("field", list(clc.HC_GUARDS))
def test_the_hot_cold_search_result_is_what_the_oracle_says(field):
    found = clc.HOT_COLD_SEARCH["fields"][field]
    cut = clc.hot_cold_cut(found["strategy"])
    assert cut["R"] == found["R"]
    if found["reachable"]:  # the next round takes this field, and no other, to its guard bit
        assert cut["crossing"] == [field]
        assert max(cut["ratios"].values()) < 1.0 and cut["ratios"][field] * clc.HC_GUARDS[field] == clc.HC_GUARDS[field] - 1
    else:
        assert field not in cut["crossing"] and round(cut["ratios"][field], 4) == found["closest"] < 1.0


def test_farkles_are_the_reachable_hot_cold_field():
    assert list(clc.hot_cold_cases()) == ["farkles"]
    case = clc.hot_cold_cases()["farkles"]
    assert case["R"] == clc.HC_GUARDS["farkles"] - 1  # a never-banking seat farkles once a round
    for k, S in ((4, 96), (8, 96)):  # the tables the GPU file plays: every seat of every game holds R farkles after R rounds
        for form in ki.FORMS:
            rows = clc.call_reference(clc.never_bank_table(form, S), k, None, call={**clc.CALL, "max_rounds": case["R"] + 1})["rows"]
            assert (rows["seats"]["farkles"] == case["R"] + 1).all()
            for name, bit in clc.HC_GUARDS.items():
                if name != "farkles":
                    assert int(rows["seats"][name].max()) < bit, (name, k, form)


def test_the_bank_at_once_table_reaches_the_largest_targets():
    for k, S, target in ((2, 96, clc.LEAN_TARGET), (3, 96, clc.LEAN_TARGET), (4, 96, clc.FULL_TARGET), (4, 96, clc.HC_TARGET),
                         (6, 96, clc.HC_TARGET), (8, 96, clc.HC_TARGET)):
        _, ref = clc.maxima_reference(k, S, target)
        scores = clc.winners_scores(ref["rows"])
        assert (scores >= target).all() and scores.max() < target + 65_500
        assert int(ref["rows"]["seats"]["rolls"].max()) < clc.MAXIMA_ROUNDS + 100  # every counter far inside its field


def test_the_trace_list_has_one_then_two_games_beyond_16_bits():
    case = clc.trace_case()
    rows = case["rows"]([0, 1, 2], case["R_in"])
    assert rows is not None and int(rows["status"][0]) == 0 and int(clc.winners_scores(rows[:1])[0]) >= clc.TRACE_TARGET
    assert clc.U16_LIMIT - 1000 < int(rows["seats"]["rolls"].max()) <= clc.U16_LIMIT
    assert int(rows["seats"]["rolls"][1].max()) == int(rows["seats"]["rolls"][2].max()) == clc.U16_LIMIT
    assert case["R_both"] == case["R_in"] + 1 and rows[1].tobytes() != rows[2].tobytes()
    assert case["rows"]([1], case["R_both"]) is None and case["rows"]([2], case["R_both"]) is None and case["rows"]([0], case["R_both"]) is not None


def test_the_census_calls_offender_is_in_the_second_chunk():
    case, cc = clc.census_case(), clc.CENSUS_CALL
    assert case["row_out"] is None and case["R_out"] == case["R_in"] + 1
    assert int(case["row_in"]["seats"]["rolls"].max()) == clc.U16_LIMIT
    assert cc["chunk_games"] <= case["game"] < 2 * cc["chunk_games"]
