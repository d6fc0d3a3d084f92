"""The game-stats stage on the CPU: the host statement of its sufficient statistics and both table builders against
`tests/golden/game_stats_vectors.json` — the reference's OWN ``_compute_k_game_stats`` and ``_rare_event_flags`` over rows it
simulated (`tools/gen_game_stats_golden.py`) — with the same schema and every value bit-equal; merge, the 2**53 guard."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import golden_util as gu  # noqa: E402
from game_stats_engine_stub import Engine as StubEngine  # noqa: E402

from farkle_ii_amd import game_stats as gs  # noqa: E402
from farkle_ii_amd.backend import make_overrides  # noqa: E402
from farkle_ii_amd.strategies import STRATEGY_DTYPE  # noqa: E402

CASES = gu.load("game_stats_vectors.json")["cases"]


def encode(table) -> dict:
    cols = {}
    for name in table.schema.names:
        cols[name] = [v.hex() if isinstance(v, float) and v == v else ("nan" if isinstance(v, float) else v)
                      for v in table.column(name).to_pylist()]
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def by_strategy(enc: dict) -> dict:
    """The reference's rows in its first-encounter order -> the documented order: ascending strategy ID, the n_players row last."""
    cols = enc["columns"]
    n = len(cols["summary_level"])
    order = sorted(range(n), key=lambda i: (cols["strategy"][i] is None, cols["strategy"][i] or 0))
    return {"schema": enc["schema"], "columns": {name: [v[i] for i in order] for name, v in cols.items()}}


def case_table(case):
    table = gu.strategies_from_tuples(case["strategies"], STRATEGY_DTYPE)
    return table, np.asarray(table["strategy_id"], dtype=np.int32)


def cell_overrides(cell):
    # fixture rows are (root, k, shuffle, game, max_rounds)
    return make_overrides((o[0], o[2], o[3], o[1], o[4]) for o in cell["overrides"]) if cell["overrides"] else None


def cell_summary(eng, case, cell, **kw) -> gs.GameStatsSummary:
    table, _ = case_table(case)
    res = eng.tournament_game_stats(table, cell["k"], case["root_seed"], 0, cell["n_shuffles"], target_score=case["target_score"],
                                    max_rounds=case["max_rounds"], overrides=cell_overrides(cell),
                                    rare_target_score=case["rare_target_score"], **kw)
    return gs.GameStatsSummary.from_engine(res, cell["k"])


def check_case(case, summaries):
    import pyarrow as pa

    _, ids = case_table(case)
    for cell, summary in zip(case["cells"], summaries):
        got = gs.game_stats_table(summary, ids, cell["k"], case["thresholds"])
        assert encode(got) == by_strategy(cell["game_stats"]), f"{case['name']} k={cell['k']}"
    rare = gs.rare_event_summary_table({c["k"]: s for c, s in zip(case["cells"], summaries)}, ids, case["thresholds"],
                                       strategy_arrow=pa.type_for_alias(case["strategy_arrow"]))
    if case["rare_event_summary"] is None:
        assert rare is None
    else:
        assert encode(rare) == case["rare_event_summary"], case["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_statement_reproduces_the_reference(case):
    eng = StubEngine()
    summaries = [cell_summary(eng, case, cell) for cell in case["cells"]]
    for cell, s in zip(case["cells"], summaries):
        assert int(s.game_counts[gs.SAFETY]) == cell["safety_limit_games"]
    check_case(case, summaries)


def test_fixture_covers_the_issue_cases():
    ks = {c["k"] for case in CASES for c in case["cells"]}
    assert {1, 2, 4, 7} <= ks
    assert any(c["safety_limit_games"] > 0 for case in CASES for c in case["cells"])
    assert any(case["pad_to"] == 12 for case in CASES)
    assert any(tuple(case["thresholds"]) != gs.DEFAULT_MARGIN_THRESHOLDS and case["rare_target_score"] != gs.DEFAULT_RARE_TARGET_SCORE
               for case in CASES)


@pytest.mark.parametrize("case", CASES[:2], ids=[c["name"] for c in CASES[:2]])
def test_merge_is_additive_over_split_ranges(case):
    eng = StubEngine()
    table, ids = case_table(case)
    for cell in case["cells"]:
        whole = cell_summary(eng, case, cell)
        k, n = cell["k"], cell["n_shuffles"]
        kw = dict(target_score=case["target_score"], max_rounds=case["max_rounds"], overrides=cell_overrides(cell),
                  rare_target_score=case["rare_target_score"])
        parts = [gs.GameStatsSummary.from_engine(eng.tournament_game_stats(table, k, case["root_seed"], a, b, **kw), k)
                 for a, b in ((0, 1), (1, n - 1), (n - 1, n))]
        for merged in (parts[0].merge(parts[1]).merge(parts[2]), parts[2].merge(parts[0].merge(parts[1]))):
            for name, a in whole.to_arrays().items():
                b = merged.to_arrays()[name]
                if name == "k":
                    assert a == b
                else:
                    n_ = max(np.shape(a)[-1], np.shape(b)[-1])
                    assert np.array_equal(gs._add_padded(np.asarray(a), np.zeros(np.shape(a)[:-1] + (n_,), np.int64)),
                                          gs._add_padded(np.asarray(b), np.zeros(np.shape(b)[:-1] + (n_,), np.int64))), name
        assert gs.game_stats_table(merged, ids, k).equals(gs.game_stats_table(whole, ids, k))


def test_merge_spills_places_every_entry():
    g = {"strategy_counts": np.zeros((3, 4), np.int64), "strategy_rounds": np.zeros((3, 4), np.int64),
         "strategy_runner": np.zeros((3, 2), np.int64), "strategy_spread": np.zeros((3, 2), np.int64),
         "game_counts": np.zeros(4, np.int64), "game_rounds": np.zeros(4, np.int64), "game_runner": np.zeros(2, np.int64)}
    spill = np.array([[0, 0, 9], [2, 1, 5], [2, 2, 7], [-1, 0, 4], [-1, 1, 3], [1, 0, 2]], np.int32)
    out = gs.merge_spills(g, spill, rounds_bins_total=12)
    assert out["strategy_rounds"].shape == (3, 12) and out["game_rounds"].shape == (12,)
    assert out["strategy_rounds"][0, 9] == 1 and out["strategy_rounds"][1, 2] == 1 and out["game_rounds"][4] == 1
    assert out["strategy_runner"].shape == (3, 8) and out["strategy_runner"][2, 5] == 1 and out["strategy_spread"][2, 7] == 1
    assert out["game_runner"][3] == 1
    with pytest.raises(ValueError):
        gs.merge_spills(g, np.array([[5, 0, 1]], np.int32), 4)


def test_float_sums_beyond_2_53_are_refused():
    def summary(value: int, times: int) -> gs.GameStatsSummary:  # one strategy, every exposure n_rounds = value
        s = gs.GameStatsSummary.empty(2, 1)
        s.strategy_counts[0] = s.game_counts[:] = [times, times, 0, 0]
        s.strategy_rounds = np.zeros((1, value + 1), np.int64)
        s.strategy_rounds[0, value] = times
        s.game_rounds = s.strategy_rounds[0].copy()
        return s

    assert gs.game_stats_table(summary(3, 2 ** 49), [7], 2) is not None  # sum of squares 9 * 2**49 < 2**53: exact
    with pytest.raises(OverflowError, match="2\\*\\*53"):
        gs.game_stats_table(summary(3, 2 ** 51), [7], 2)  # 9 * 2**51 > 2**53: the reference's float64 sum rounds
