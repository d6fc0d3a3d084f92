"""The inputs of ``test_wide_tables_gpu.py`` reach the regimes they are there for — shown on the oracle's result and on the
sources' constants alone, without a GPU: every case has completed and safety-limit games (each at least 5 % of its games), wins
at seat 0 and at the last seat, a ragged last batch; the 128-seat case wins at seats beyond 63 and at seat 127; the rare-event
lists are not empty; the launch plan and the rows tile restated from ``LDS_LIMIT``, the record sizes and the tile size give the
shape each player count is named for; the oracle plays 128 seats and refuses 129."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import wide_table_cases as wt
from oracle_engine_stub import po
from rare_events_engine_stub import Engine as RareStub

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("k", wt.KS)
def test_case_reaches_both_outcomes_and_both_ends_of_the_table(k):
    fig = wt.check_preconditions(k)
    print(k, fig)
    assert fig["games"] == {13: 320, 16: 320, 17: 320, 19: 120, 32: 120, 33: 120, 37: 80, 38: 80, 64: 400, 65: 400, 128: 600}[k]
    if k == 128:
        assert (fig["safety"], fig["last_seat_wins"]) == (115, 5)  # (what the oracle gave when the case was chosen)


@pytest.mark.parametrize("k", wt.POST_PASS_KS)
def test_rare_event_list_is_not_empty(k):
    want = RareStub().tournament_rare_events(wt.table(k), k, thresholds=wt.RARE_THRESHOLDS, **wt.call(k))
    n = want["rare_events"]["events"]
    print(k, "events", n, "of", n_games := wt.figures(k)["games"])
    assert 0 < n < n_games


def test_the_limit_is_one_constant_of_the_header_and_of_the_oracle():
    header = (ROOT / "include" / "farkle_hip.h").read_text()
    assert [int(v) for v in re.findall(r"#define FK_MAX_PLAYERS (\d+)", header)] == [wt.MAX_PLAYERS]
    oracle = (ROOT / "oracle" / "farkle_oracle.c").read_text()
    assert [int(v) for v in re.findall(r"#define FKO_MAX_K (\d+)", oracle)] == [wt.MAX_PLAYERS]
    # an int8 winner seat with -1 for none, a uint8 rank from 1, seven seat bits under the safety flag of the result word
    assert wt.MAX_PLAYERS - 1 == np.iinfo(np.int8).max and wt.MAX_PLAYERS <= np.iinfo(np.uint8).max
    assert ((wt.MAX_PLAYERS - 1) << 24) < 0x80000000 <= (wt.MAX_PLAYERS << 24)


def test_oracle_plays_128_seats_and_refuses_129():
    assert len(wt.want(128)["rows"]) == 600 and wt.want(128)["rows"].dtype.itemsize == 4 + 28 * 128
    t = wt.ki._random_legal(129, 1).view(po.STRATEGY_DTYPE)
    with pytest.raises(po.OracleError):
        po.tournament(t, 129, wt.ROOT, 0, 1)
    coords = np.array([po.coord(102, wt.ROOT, k=129)], dtype=po.COORD_DTYPE).reshape(-1)
    with pytest.raises(po.OracleError):
        po.play_games(coords, t, np.arange(129, dtype=np.int32), 129)
    coords128 = np.array([po.coord(102, wt.ROOT, k=128)], dtype=po.COORD_DTYPE).reshape(-1)
    assert len(po.play_games(coords128, t[:128], np.arange(128, dtype=np.int32), 128)) == 1


# ----------------------------------------------------------------------- the table of shapes, restated from the constants
def test_constants_are_the_ones_the_table_of_shapes_was_worked_out_with():
    c = wt.constants()
    assert (c["LDS_LIMIT"], c["LEAN_BYTES"], c["FULL_BYTES"], c["ROWS_TILE"], c["ROWS_FIRST_BLOCK"]) == (163_840, 40, 68, 65_536, 256)
    assert c["HC_MAX_K"] == 12 and 50 * c["LEAN_MAX_TARGET50"] == wt.BEYOND_LEAN - 1
    assert min(wt.KS) == c["HC_MAX_K"] + 1  # the first count past the hot / cold kernel


# k -> block, lean records, state-store instance, dynamic LDS bytes of the default plan of a multi-batch call
DEFAULT_PLAN = {13: (256, True, False, 133_120), 16: (256, True, False, 163_840), 17: (64, True, False, 43_520),
                19: (64, True, False, 48_640), 32: (128, True, False, 163_840), 33: (64, False, False, 143_616),
                37: (64, False, False, 161_024), 38: (64, True, False, 97_280), 64: (64, True, False, 163_840),
                65: (768, True, True, 30_720), 128: (768, True, True, 30_720)}


@pytest.mark.parametrize("k", wt.KS)
def test_default_plan_of_each_player_count(k):
    p = wt.plan(k, wt.table_size(k))
    assert (p["block"], p["lean"], p["gs"], p["lds"]) == DEFAULT_PLAN[k]
    c = wt.constants()
    if not p["gs"]:
        assert p["lds"] == p["block"] * k * (c["LEAN_BYTES"] if p["lean"] else c["FULL_BYTES"])
    assert (p["lds"] == c["LDS_LIMIT"]) == (k in (16, 32, 64))  # LDS filled to the byte
    assert (p["per_cu"] == 3) == (k in (17, 19)) and (k != 64 or (p["block"], p["per_cu"]) == (64, 1))  # one wave per CU at 64


def test_plan_boundaries():
    c = wt.constants()
    full, lean, limit = c["FULL_BYTES"], c["LEAN_BYTES"], c["LDS_LIMIT"]
    # 33 .. 37: full and lean records seat the same 64 lanes per CU, the tie goes to full records; 37 is the last that fits
    for k in (33, 37):
        assert wt.plan(k, 2 * k, lean=1)["per_cu"] * 64 == wt.plan(k, 2 * k, lean=0)["per_cu"] * 64 == 64
    assert 64 * 37 * full <= limit < 64 * 38 * full
    assert wt.plan(32, 96, lean=0) == dict(block=64, lean=False, gs=False, lds=64 * 32 * full, tally=False, per_cu=1)
    # 38 with lean = 0: the state-store instance; with a target beyond lean records: no instance at 38, full records at 37
    assert wt.plan(38, 76, lean=0)["gs"] and wt.plan(38, 76, lean=1) == wt.plan(38, 76)
    assert wt.plan(38, 76, target_score=wt.BEYOND_LEAN) is None
    assert wt.plan(37, 74, target_score=wt.BEYOND_LEAN)["lean"] is False and wt.plan(37, 74, target_score=wt.BEYOND_LEAN - 1)["lean"] is False
    assert wt.plan(38, 76, target_score=wt.BEYOND_LEAN - 1)["lean"] is True
    # 64 is the last count whose lean records fit; 65 .. 128 play on the state-store instance whatever `lean` says
    assert 64 * 64 * lean == limit < 64 * 65 * lean
    for k in (65, 128):
        assert all(wt.plan(k, wt.table_size(k), lean=v)["gs"] for v in (-1, 0, 1))
    # state_store = 1 takes every case to the same instance
    assert all(wt.plan(k, wt.table_size(k), state_store=1) == dict(wt.plan(128, 128), per_cu=2) for k in wt.KS)


# k -> block, lean records, state-store instance, LDS tally of a counts-only call of ONE batch: a block takes the tally whenever it
# fits beside its records, which moves 17 and 19 to 128-thread blocks, fills LDS to 162 624 bytes at 33 (full records + tally) and
# flips 37 to lean records (full ones leave no room for the tally, and the tally wins the tie)
ONE_BATCH_PLAN = {13: (256, True, False, True), 16: (256, True, False, False), 17: (128, True, False, True), 19: (128, True, False, True),
                  32: (128, True, False, False), 33: (64, False, False, True), 37: (64, True, False, True), 38: (64, True, False, True),
                  64: (64, True, False, False), 65: (768, True, True, True), 128: (768, True, True, True)}


def test_one_batch_calls_decide_on_an_lds_tally_beside_the_records():
    """A counts-only call of one batch may keep its tally in LDS: beside records that fill LDS to the byte there is no room for it."""
    c = wt.constants()
    for k in wt.KS:
        S = wt.table_size(k)
        multi, one = wt.plan(k, S), wt.plan(k, S, single_batch=True)
        tally_bytes = S * c["LT_COLS"] * 8
        assert one["lds"] == wt.record_lds_bytes(k, one["block"], one["lean"], one["gs"], False, S) + (tally_bytes if one["tally"] else 0)
        if multi["lds"] == c["LDS_LIMIT"]:
            assert not one["tally"] and one == multi, k  # 16, 32, 64: the records leave no byte for it
        assert (one["block"], one["lean"], one["gs"], one["tally"]) == ONE_BATCH_PLAN[k], k
        assert wt.plan(k, S, single_batch=True, use_lds_tally=0) == multi


def test_rows_tile_of_each_player_count():
    assert {k: wt.rows_tile_lanes(k) for k in wt.KS} == {13: 128, 16: 128, 17: 128, 19: 64, 32: 64, 33: 64, 37: 0, 38: 0, 64: 0, 65: 0, 128: 0}
    assert wt.rows_tile_lanes(12) == 192 and wt.rows_tile_lanes(18) == 128  # 128 lanes while 4 + 28 k <= 512 bytes
    assert wt.rows_tile_lanes(36) == 64 and 4 + 28 * 36 <= 1024 < 4 + 28 * 37


def test_column_kernels_and_narrower_limits():
    hip = (wt.CSRC / "farkle_hip.hip").read_text()
    assert "if (columns && k <= 16 && c->columns_by_seat != 0)" in hip  # up to sixteen seats: 64 k <= 1 024 threads per (game, seat)
    assert 64 * 13 == 832 and 64 * 16 == 1024
    assert re.findall(r"constexpr uint32_t MAX_K = (\d+);", (wt.CSRC / "fk_seat_analysis.h").read_text()) == ["16"]
    assert re.findall(r"constexpr uint32_t MAX_K = (\d+);", (wt.CSRC / "fk_matchups.h").read_text())[:1] == ["16"]
    assert max(wt.COLUMN_KS) == 64 and "column images hold tables of at most 64 seats" in hip
