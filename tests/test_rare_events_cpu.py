"""The rare-event game rows and quantile thresholds on the CPU: the host statement (``farkle_ii_amd.rare_events``) over the oracle's
rows against `tests/golden/rare_events_vectors.json` — the reference's OWN ``_resolve_rare_event_thresholds``,
``_build_rare_event_summary_shard`` (with the batch lengths its reader produced), ``_rare_event_details`` and ``_rare_event_flags``
over rows it simulated (`tools/gen_rare_events_golden.py`).  Tables are compared by schema (names and Arrow types), row order and
every value with floats by bits (``float.hex``; ``Table.equals`` itself calls two NaN margins different, so the encoded form stands
in for it wherever a table holds a safety-limit game)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import golden_util as gu  # noqa: E402
from rare_events_engine_stub import Engine as StubEngine  # noqa: E402
from test_game_stats_cpu import case_table, cell_overrides, encode  # noqa: E402

from farkle_ii_amd import game_stats as gs  # noqa: E402
from farkle_ii_amd import rare_events as rev  # noqa: E402

CASES = gu.load("rare_events_vectors.json")["cases"]


def same_table(got, want_encoded: dict, what: str) -> None:
    """Schema, order and every value (floats by bits) against a recorded table."""
    enc = encode(got)
    assert enc["schema"] == want_encoded["schema"], what
    for name, column in want_encoded["columns"].items():
        if isinstance(column, dict):  # the fixture stores columns with long runs as (value, count) pairs
            column = [v for v, n in column["runs"] for _ in range(n)]
        assert enc["columns"][name] == column, f"{what}: column {name}"


def cell_call(eng, case, cell, rare_target, thresholds, want_events=True, **kw) -> dict:
    table, _ = case_table(case)
    return eng.tournament_rare_events(table, cell["k"], case["root_seed"], 0, cell["n_shuffles"], target_score=case["target_score"],
                                      max_rounds=case["max_rounds"], overrides=cell_overrides(cell), rare_target_score=rare_target,
                                      thresholds=thresholds, want_events=want_events, **kw)


def check_case(case, eng) -> None:
    """The whole chain of one fixture case through ``eng.tournament_rare_events``: histograms -> resolved thresholds -> events ->
    the three tables."""
    import pyarrow as pa

    table, ids = case_table(case)
    arrow = pa.type_for_alias(case["strategy_arrow"])
    quantile = case["margin_quantile"] is not None or case["target_rate"] is not None
    first = {c["k"]: cell_call(eng, case, c, case["rare_target_score"], () if quantile else case["thresholds"], want_events=not quantile)
             for c in case["cells"]}
    summaries = {k: rev.RareEventSummary.from_engine(r, k) for k, r in first.items()}
    for s in summaries.values():
        assert rev.tail_equals_multi_target(s, case["rare_target_score"])
    thr, target = rev.resolve_rare_event_thresholds(summaries, case["thresholds"], case["rare_target_score"], case["margin_quantile"],
                                                    case["target_rate"])
    assert list(thr) == case["resolved_thresholds"] and target == case["resolved_target_score"], case["name"]
    second = {c["k"]: cell_call(eng, case, c, target, thr) for c in case["cells"]} if quantile else first
    events = {}
    for cell in case["cells"]:
        k = cell["k"]
        r = second[k]
        assert np.array_equal(r["tally"], first[k]["tally"])  # the replay plays the same games
        gps = len(table) // k
        head, seats = r["rare_events"]["event_head"], r["rare_events"]["event_seats"]
        events[k] = (head, seats, gps, cell["n_games"])
        assert cell["n_games"] == gps * cell["n_shuffles"]
        shard = rev.rare_event_game_table(head, seats, k, gps, cell["n_games"], ids, thr, details=False, batch_games=cell["shard_batches"],
                                          strategy_arrow=arrow)
        same_table(shard, cell["shard"], f"{case['name']} k={k} shard")
        # the shard's counters are the summary sums under the resolved values
        under = summaries[k].under_target(target)
        want = cell["shard_global_sums"]
        g = under.game_counts
        assert [int(g[gs.ATTEMPTED]), int(g[gs.COMPLETED]), int(g[gs.SAFETY]), int(g[gs.MULTI_TARGET])] == [
            want["observations"], want["completed_observations"], want["safety_limit_observations"], want["multi_reached_target"]]
        for t in thr:
            assert gs._margin_le(under.game_runner, t) == want[f"margin_le_{t}"]
        per = cell["shard_strategy_sums"]
        assert per["strategy"] == sorted(int(ids[i]) for i in np.flatnonzero(under.strategy_counts[:, gs.ATTEMPTED] > 0))
        for sid, values in zip(per["strategy"], per["values"]):
            sums = dict(zip(per["fields"], values))
            i = int(np.flatnonzero(ids == int(sid))[0])
            assert int(under.strategy_counts[i, gs.MULTI_TARGET]) == sums["multi_reached_target"]
            assert int(under.strategy_counts[i, gs.ATTEMPTED]) == sums["observations"]
            assert int(under.strategy_counts[i, gs.COMPLETED]) == sums["completed_observations"]
            assert int(under.strategy_counts[i, gs.SAFETY]) == sums["safety_limit_observations"]
            for t in thr:
                assert gs._margin_le(under.strategy_runner[i], t) == sums[f"margin_le_{t}"]
    details = rev.rare_event_details_table(events, ids, thr, batch_games={c["k"]: c["details_batches"] for c in case["cells"]},
                                           strategy_arrow=arrow)
    if case["details"] is None:
        assert details is None
    else:
        same_table(details, case["details"], f"{case['name']} details")
    final = rev.rare_events_table(events, summaries, ids, thr, target, batch_games={c["k"]: c["flags_batches"] for c in case["cells"]},
                                  strategy_arrow=arrow)
    if case["rare_events"] is None:
        assert final is None
    else:
        same_table(final, case["rare_events"], f"{case['name']} rare_events")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_statement_reproduces_the_reference(case):
    check_case(case, StubEngine())


def test_fixture_covers_the_issue_cases():
    ks = {c["k"] for case in CASES for c in case["cells"]}
    assert {1, 2, 4, 7} <= ks
    assert any(case["pad_to"] == 12 for case in CASES)
    assert any(len(case["thresholds"]) == 3 for case in CASES)
    modes = {(case["margin_quantile"] is not None, case["target_rate"] is not None) for case in CASES}
    assert modes == {(False, False), (True, False), (False, True), (True, True)}
    assert any(case["rare_target_score"] < case["target_score"] and case["classes"]["flagged_safety_limit"] > 0 for case in CASES)
    for name in ("multi_only", "margin_only", "both", "flagged_safety_limit", "unflagged"):
        assert sum(case["classes"][name] for case in CASES) >= 1, name
    assert any(len(c["shard_batches"]) >= 2 for case in CASES for c in case["cells"])


def _events(head, seats, k, gps, n_games, ids, thr, **kw):
    return rev.rare_event_game_table(head, seats, k, gps, n_games, ids, thr, **kw)


def test_both_batchings_order_the_same_rows_differently():
    """One batch is plain seat-major; the reader's small batches are seat-major inside each batch — the same multiset of rows."""
    case = next(c for c in CASES if c["name"] == "k1247")
    cell = next(c for c in case["cells"] if c["k"] == 4)
    table, ids = case_table(case)
    r = cell_call(StubEngine(), case, cell, case["resolved_target_score"], case["resolved_thresholds"])
    head, seats = r["rare_events"]["event_head"], r["rare_events"]["event_seats"]
    gps = len(table) // 4
    thr = case["resolved_thresholds"]
    one = _events(head, seats, 4, gps, cell["n_games"], ids, thr, details=True, batch_games=65_536)
    many = _events(head, seats, 4, gps, cell["n_games"], ids, thr, details=True, batch_games=cell["shard_batches"])
    fixed = _events(head, seats, 4, gps, cell["n_games"], ids, thr, details=True, batch_games=4)
    n = len(head)
    assert one.num_rows == many.num_rows == fixed.num_rows == 4 * n and n > 4
    assert one.column("strategy").to_pylist() == [int(ids[s]) for s in seats.T.reshape(-1)]  # P1 of every game, then P2 ...
    assert one.column("strategy").to_pylist() != many.column("strategy").to_pylist()
    key = lambda t: sorted(zip(*[[str(v) for v in t.column(c).to_pylist()] for c in t.schema.names]))  # noqa: E731
    assert key(one) == key(many) == key(fixed)
    with pytest.raises(ValueError):
        _events(head, seats, 4, gps, cell["n_games"], ids, thr, details=True, batch_games=[cell["n_games"] - 1])


def test_details_and_shard_forms_differ_only_in_types():
    import pyarrow as pa

    case = next(c for c in CASES if c["name"] == "safety_limit")
    cell = case["cells"][0]
    table, ids = case_table(case)
    r = cell_call(StubEngine(), case, cell, case["resolved_target_score"], case["resolved_thresholds"])
    args = (r["rare_events"]["event_head"], r["rare_events"]["event_seats"], cell["k"], len(table) // cell["k"], cell["n_games"], ids,
            case["resolved_thresholds"])
    shard, details = _events(*args, details=False), _events(*args, details=True)
    assert shard.schema.field("multi_reached_target").type == pa.float64() and details.schema.field("multi_reached_target").type == pa.uint8()
    assert shard.schema.field("observations").type == details.schema.field("observations").type == pa.uint8()
    assert shard.schema.field("n_players").type == pa.int32() and shard.schema.field("termination_status").type == pa.string()
    assert encode(shard.cast(details.schema))["columns"] == encode(details)["columns"]
    status = details.column("termination_status").to_pylist()
    margin = details.column("margin_runner_up").to_pylist()
    assert "safety_limit" in status and all((m != m) == (s == "safety_limit") for m, s in zip(margin, status))


def _summary(k, runner=(), second=()) -> rev.RareEventSummary:
    s = gs.GameStatsSummary.empty(k, 1)
    s.game_runner = np.asarray(list(runner) or [0], np.int64)
    return rev.RareEventSummary(s, np.zeros((1, 1), np.int64), np.asarray(list(second) or [0], np.int64))


def test_resolve_thresholds_edges():
    fixed = rev.resolve_rare_event_thresholds({2: _summary(2, [1, 2])}, (500, 1000), 10_000, None, None)
    assert fixed == ((500, 1000), 10_000)
    # an empty histogram leaves the configured values
    assert rev.resolve_rare_event_thresholds({2: _summary(2)}, (500, 1000), 10_000, 0.5, 0.5) == ((500, 1000), 10_000)
    # all mass in one bin: every quantile is that bin
    one = {2: _summary(2, [0, 0, 0, 9], [0] * 7 + [4])}
    for q in (1e-9, 0.5, 1 - 1e-9):
        assert rev.resolve_rare_event_thresholds(one, (500, 1000), 10_000, q, q) == ((150,), 350)
    # the quantile landing exactly on a cumulative count: cutoff = ceil(total q) = that count, so the bin that reaches it
    steps = {2: _summary(2, [2, 2, 4, 2]), 3: _summary(3, [0, 0, 0, 0, 10])}  # pooled cumulative 2, 4, 8, 10, 20
    assert rev.resolve_rare_event_thresholds(steps, (500,), 10_000, 0.2, None) == ((50,), 10_000)     # cutoff 4 -> bin 1
    assert rev.resolve_rare_event_thresholds(steps, (500,), 10_000, 0.25, None) == ((100,), 10_000)   # cutoff 5 -> bin 2
    assert rev.resolve_rare_event_thresholds(steps, (500,), 10_000, 0.4, None) == ((100,), 10_000)    # cutoff 8 -> bin 2
    assert rev.resolve_rare_event_thresholds(steps, (500,), 10_000, 0.5, None) == ((150,), 10_000)    # cutoff 10 -> bin 3
    assert rev.resolve_rare_event_thresholds(steps, (500,), 10_000, 0.500001, None) == ((200,), 10_000)
    # the target is the 1 - rate quantile of the pooled second scores; the thresholds stay when only the rate is given
    sec = {2: _summary(2, [5], [0, 6, 0, 2]), 4: _summary(4, [5], [0, 0, 2])}  # cumulative 6, 8, 10 at bins 1, 2, 3
    assert rev.resolve_rare_event_thresholds(sec, (500, 1000), 10_000, None, 0.2) == ((500, 1000), 100)  # q = 0.8 -> cutoff 8
    assert rev.resolve_rare_event_thresholds(sec, (500, 1000), 10_000, None, 0.1) == ((500, 1000), 150)  # q = 0.9 -> cutoff 9
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="rare_event_margin_quantile must be between 0 and 1"):
            rev.resolve_rare_event_thresholds(sec, (500,), 10_000, bad, None)
        with pytest.raises(ValueError, match="rare_event_target_rate must be between 0 and 1"):
            rev.resolve_rare_event_thresholds(sec, (500,), 10_000, None, bad)


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_tail_of_the_second_histograms_is_the_multi_target_count(k):
    from tools.time_config import table_for

    t = table_for(60)
    eng = StubEngine()
    rows = eng.tournament(t, k, 42, 0, 6, want_rows=True, target_score=3000)["rows"]
    for target in (-50, 0, 1, 50, 1975, 2000, 2950, 3000, 3050, 100_000):
        s = rev.RareEventSummary.from_rows(rows, k, len(t), target)
        assert rev.tail_equals_multi_target(s, target), target
        other = rev.RareEventSummary.from_rows(rows, k, len(t), 10_000).under_target(target)  # any launch target gives the same tail
        assert np.array_equal(other.strategy_counts, s.stats.strategy_counts) and np.array_equal(other.game_counts, s.stats.game_counts)
    if k == 1:
        assert s.game_second.sum() == 0
    else:
        assert s.game_second.sum() == len(rows) and np.all(s.strategy_second.sum(axis=1) == 6)


def test_events_of_split_ranges_concatenate_and_spills_merge():
    from tools.time_config import table_for

    t = table_for(64)
    eng = StubEngine()
    kw = dict(target_score=3000, rare_target_score=2000, thresholds=(100, 500))
    whole = eng.tournament_rare_events(t, 4, 9, 10, 40, **kw)["rare_events"]
    parts = [eng.tournament_rare_events(t, 4, 9, a, b, **kw)["rare_events"] for a, b in ((10, 11), (11, 30), (30, 40))]
    head, seats = rev.concat_events([(p["event_head"], p["event_seats"]) for p in parts], [0, 1, 20])
    assert 0 < len(head) < 30 * 16 and np.array_equal(head, whole["event_head"]) and np.array_equal(seats, whole["event_seats"])
    per, game = rev.merge_second_spills(np.zeros((3, 2), np.int64), np.zeros(2, np.int64),
                                        np.array([[-1, 3, 7], [2, 3, 5], [2, 3, 5], [0, 3, 1]], np.int32))
    assert per.shape == (3, 8) and game.shape == (8,) and game[7] == 1 and per[2, 5] == 2 and per[0, 1] == 1 and per.sum() == 3
    with pytest.raises(ValueError):
        rev.merge_second_spills(np.zeros((3, 2), np.int64), np.zeros(2, np.int64), np.array([[3, 3, 1]], np.int32))
