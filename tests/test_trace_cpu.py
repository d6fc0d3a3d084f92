"""What sits on top of the device's roll-level trace, without a GPU: the events come from tests/trace_oracle.py (the CPU oracle's
game loop restated on its own primitives and pinned, in every case, by `row == the oracle's row`), the expected messages from the
reference's own ``watch_game`` and tracing wrappers (tests/golden/watch_vectors.json, tools/gen_watch_golden.py)."""
from __future__ import annotations

import hashlib
import logging
import re
from pathlib import Path

import golden_util as gu
import numpy as np
import pyoracle as po
import pytest
import trace_oracle
from trace_engine_stub import TraceEngineStub

from farkle_ii_amd import trace, watch_game as wg
from farkle_ii_amd.backend import EVENT_DTYPE, make_coords
from farkle_ii_amd.strategies import STRATEGY_DTYPE, pack_strategies

ROOT = Path(__file__).resolve().parent.parent
VECTORS = gu.load("watch_vectors.json")
WATCH = {case["seed"]: case for case in VECTORS["watch"]}


def digest(messages) -> str:
    return hashlib.sha256("\n".join(messages).encode()).hexdigest()


def watch_messages(seed: int) -> list[str]:
    """`render` over the helper's events of the watch_game(seed) game."""
    strategies = wg.watch_strategies(seed)
    table = pack_strategies(strategies)
    assert [list(t)[:10] for t in table.tolist()] == [t[:10] for t in WATCH[seed]["strategies"]]
    rows, begin, events = trace_oracle.pinned(make_coords(10, seed, 2), table, [0, 1], 2)
    return wg.render(events, strategies, rows[0])


@pytest.mark.parametrize("seed", [47, 6, 42, 12, 25])
def test_render_equals_the_reference_messages(seed):
    assert watch_messages(seed) == WATCH[seed]["messages"]


def test_final_turn_overtake_has_no_decide_line():
    for seed in (12, 25):
        rolls = [m for m in WATCH[seed]["messages"] if not m.startswith(("Winner", "\n====="))]
        assert rolls[-1].startswith("score(")
    assert any("reroll=0" in a and "dice_left=6" in b for a, b in zip(WATCH[25]["messages"], WATCH[25]["messages"][1:]))


def test_render_matches_count_and_digest_of_the_long_games():
    mine = watch_messages(7)
    assert (len(mine), digest(mine)) == (WATCH[7]["count"], WATCH[7]["sha256"]) and WATCH[7]["count"] == 482
    # seed 253: 200 rounds without a winner; the reference cannot format its last record, ours is spelled out
    mine = watch_messages(253)
    assert WATCH[253]["truncated"] and mine[-2] == wg.FINAL_RESULT and mine[-1] == "Winner: None  score=None  rounds=200"
    assert (len(mine) - 1, digest(mine[:-1])) == (WATCH[253]["count"], WATCH[253]["sha256"])
    assert sum(m.startswith("score(") for m in mine) == 1727


@pytest.mark.parametrize("case", VECTORS["scripted"], ids=lambda c: c["name"])
def test_scripted_flag_games_equal_the_reference_messages(case):
    table = gu.strategies_from_tuples(case["strategies"], STRATEGY_DTYPE)
    coords = make_coords(case["purpose"], case["root_seed"], case["k"], shuffle_index=case["shuffle"], game_index=case["game"])
    rows, begin, events = trace_oracle.pinned(coords, table, list(range(case["k"])), case["k"], case["target"], case["max_rounds"])
    assert wg.render_rolls(events) == case["messages"]
    assert rows[0]["seats"]["score"].tolist() == case["outcome"]["scores"] and int(rows[0]["n_rounds"]) == case["outcome"]["n_rounds"]
    assert rows[0]["seats"]["rolls"].tolist() == case["outcome"]["rolls"]
    if case["name"] == "auto_hot_dice":
        assert int(trace.auto_hot(events).sum()) == case["seen"]["hot_dice"] > 0
    else:
        assert int(((trace.d5(events) > 0).astype(int) + (trace.d1(events) > 0)).sum()) == case["seen"]["discards"] > 0
        above = trace.final_round(events) & trace.decided(events) & trace.rolls_again(events)
        assert case["seen"]["run_ups"] > 0 and above.any()


def random_table(rs, n: int) -> np.ndarray:
    """Random valid strategies with extreme thresholds among them."""
    table = np.zeros(n, dtype=STRATEGY_DTYPE)
    for i in range(n):
        sf = int(rs.integers(0, 2))
        so = int(rs.integers(0, 2)) if sf else 0
        cs, cd = int(rs.integers(0, 2)), int(rs.integers(0, 2))
        rb = int(rs.integers(0, 2)) if cs and cd else 0
        thr = int(rs.choice([-(2**31), -1, 0, 1, 49, 50, 51, 200, 300, 350, 500, 1000, 1001, 2500, 10_000, 2**31 - 1]))
        table[i] = (thr, int(rs.choice([-128, -1, 0, 1, 2, 3, 4, 5, 6, 127])), sf, so, cs, cd, rb, int(rs.integers(0, 2)), int(rs.integers(0, 2)),
                    int(rs.integers(0, 2)), 1000 + i)
    return table


def test_rows_from_events_equal_the_oracle_rows_on_500_games():
    rs = np.random.default_rng(20260)
    table = random_table(rs, 96)
    games = 0
    for k in range(1, 13):
        for target, max_rounds, n in ((100, 200, 8), (2000, 200, 14), (10_000, 200, 6), (2000, 3, 8), (10_000, 0, 3), (100, 3, 3)):
            coords = make_coords(int(rs.choice([10, 103])), int(rs.integers(0, 2**63)), k, shuffle_index=rs.integers(0, 10**6, size=n),
                                 game_index=rs.integers(0, 3000, size=n))
            ss = rs.integers(0, len(table), size=(n, k))
            rows, begin, events = trace_oracle.pinned(coords, table, ss, k, target, max_rounds)
            rebuilt = trace.rows_from_events(events, begin, ss, k, target, max_rounds)
            assert rebuilt.tobytes() == rows.tobytes(), (k, target, max_rounds)
            trace.check(events, begin, rows, ss, k, target, max_rounds)
            assert int(begin[-1]) == int(rows["seats"]["rolls"].sum()) and (max_rounds > 0 or begin[-1] == 0)
            games += n
    assert games >= 500


def test_check_names_the_game_seat_and_field_of_a_flipped_byte():
    table = gu.strategies_from_tuples(VECTORS["scripted"][1]["strategies"], STRATEGY_DTYPE)
    coords = make_coords(103, 5, 3, shuffle_index=0, game_index=np.arange(4))
    ss = np.tile(np.arange(3), (4, 1))
    rows, begin, events = trace_oracle.pinned(coords, table, ss, 3, 2000)
    trace.check(events, begin, rows, ss, 3, 2000)
    # a discarded five more in one roll of game 2
    idx = next(i for i in range(int(begin[2]), int(begin[3])) if trace.d5(events[i:i + 1])[0] == 0 and events[i]["points"] > 0)
    seat = int(events[idx]["seat"])
    bad = events.copy()
    bad.view(np.uint8).reshape(-1, 16)[idx, 14] ^= 1
    with pytest.raises(ValueError, match=rf"game 2 seat {seat}: smart_five_uses is \d+ in the row, \d+ from the events"):
        trace.check(bad, begin, rows, ss, 3, 2000)
    # a farkle turned into points: the seat's farkle count is the first field to differ
    idx = next(i for i in range(int(begin[1]), int(begin[2])) if events[i]["points"] == 0)
    seat = int(events[idx]["seat"])
    bad = events.copy()
    bad.view(np.uint8).reshape(-1, 16)[idx, 8] ^= 50
    with pytest.raises(ValueError, match=rf"game 1 seat {seat}: farkles is"):
        trace.check(bad, begin, rows, ss, 3, 2000)


@pytest.fixture
def stub_engine():
    from farkle_ii_amd import engine

    stub = TraceEngineStub()
    engine.set_engine(stub)
    yield stub
    engine.set_engine(None)


def test_cli_watch_logs_the_golden_messages(stub_engine, caplog):
    from farkle_ii_amd.cli import build_parser, main

    with caplog.at_level(logging.INFO, logger="farkle_ii_amd.watch_game"):
        main(["watch", "--seed", "47"])
    records = [r for r in caplog.records if r.name == "farkle_ii_amd.watch_game"]
    assert [r.getMessage() for r in records] == WATCH[47]["messages"] and all(r.stage == "watch" for r in records)
    assert stub_engine.calls == 1
    for refused in ("analyze", "two-seed-pipeline"):
        assert build_parser().parse_args([refused]).command == refused
        with pytest.raises(SystemExit, match="outside the simulation path"):
            main([refused])


def test_cli_watch_replays_a_tournament_game_of_the_configs_grid(stub_engine, caplog, tmp_path):
    from farkle_ii_amd.cli import main

    cfg = tmp_path / "cfg.yaml"
    cfg.write_text((ROOT / "configs" / "bench_config2.yaml").read_text())
    with caplog.at_level(logging.INFO, logger="farkle_ii_amd.watch_game"):
        main(["watch", "--config", str(cfg), "--players", "2", "--shuffle", "3", "--game", "5"])
    messages = [r.getMessage() for r in caplog.records if r.name == "farkle_ii_amd.watch_game"]
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    app = load_app_config(cfg, seed_list_len=None)
    app.sim.populate_seed_list(1)
    strategies, S = runner._resolve_strategies(app, None)
    seats = po.permutation(po.coord(101, app.sim.seed, 2, 3), S)[10:12].tolist()
    assert [int(re.search(r"strategy_id\s*: (\d+)", m).group(1)) for m in messages[:2]] == [strategies[i].strategy_id for i in seats]
    row = po.play_game(po.coord(103, app.sim.seed, 2, 3, game_index=5), pack_strategies(strategies).view(po.STRATEGY_DTYPE), seats)[0]
    assert messages[-1] == f"Winner: P{row['winner_seat'] + 1}  score={row['seats'][row['winner_seat']]['score']}  rounds={row['n_rounds']}"
    with pytest.raises(SystemExit, match="needs --players, --shuffle and --game"):
        main(["watch", "--config", str(cfg), "--players", "2"])


def test_watch_game_requires_a_seed():
    with pytest.raises(ValueError, match="watch_game requires an explicit seed"):
        wg.watch_game(None)
    from farkle_ii_amd.cli import main

    with pytest.raises(ValueError, match="watch_game requires an explicit seed"):
        main(["watch"])


def test_trace_tournament_game_reproduces_the_expected_rows():
    """The reference's own EXPECTED_ROWS (tests/integration/test_raw_simulation_oracle.py:45-58), replayed by their coordinates."""
    data = gu.load("tournament_vectors.json")
    grid4 = gu.strategies_from_tuples(gu.load("grid_vectors.json")["oracle4"], STRATEGY_DTYPE)
    stub = TraceEngineStub()
    assert len(data["EXPECTED_ROWS"]) == 12
    for (root, k, shuffle, game), (seat_strats, status, winner_strategy, n_rounds, n_turns, scores) in data["EXPECTED_ROWS"]:
        max_rounds = 0 if (root, k, shuffle, game) == (11, 2, 0, 0) else 200  # the profile's one override
        row, events, seats = trace.trace_tournament_game(stub, grid4, root, k, shuffle, game, target_score=100, max_rounds=max_rounds)
        assert seats.tolist() == seat_strats == row["seats"]["strategy"].tolist()
        assert ("completed", "safety_limit")[int(row["status"])] == status
        w = int(row["winner_seat"])
        assert (None if w < 0 else int(row["seats"][w]["strategy"])) == winner_strategy
        assert int(row["n_rounds"]) == n_rounds and int(row["seats"]["n_turns"].sum()) == n_turns
        assert row["seats"]["score"].tolist() == scores and len(events) == int(row["seats"]["rolls"].sum())
        rebuilt = trace.rows_from_events(events, [0, len(events)], seats, k, 100, max_rounds)
        assert rebuilt[0].tobytes() == row.tobytes()


def test_event_dtype_has_the_headers_layout():
    header = (ROOT / "include" / "farkle_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} fk_roll_event;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(u?int(?:8|16|32)_t)\s+(\w+);", body)
    size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "int32_t": 4}
    code = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "int32_t": "<i4"}
    assert EVENT_DTYPE.itemsize == 16 and [name for _, name in fields] == list(EVENT_DTYPE.names)
    offset = 0
    for ctype, name in fields:
        offset = (offset + size[ctype] - 1) // size[ctype] * size[ctype]  # natural alignment, as the C compiler lays it out
        assert EVENT_DTYPE.fields[name][1] == offset and EVENT_DTYPE.fields[name][0] == np.dtype(code[ctype]), name
        offset += size[ctype]
    assert offset == 16
    flags = dict(re.findall(r"#define FK_EV_(\w+) (\d+)", header))
    assert {k: int(v) for k, v in flags.items()} == {"DECIDE": trace.EV_DECIDE, "ROLL_AGAIN": trace.EV_ROLL_AGAIN,
                                                     "FINAL_ROUND": trace.EV_FINAL_ROUND, "AUTO_HOT": trace.EV_AUTO_HOT}
