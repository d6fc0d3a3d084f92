"""The seat-analysis stage on the CPU: the host statement of its counts and mirrored pairs and every frame builder against
`tests/golden/seat_analysis_vectors.json` — the reference's OWN ``_iter_seat_count_tables``, ``_within_k_frames``,
``_standardized_frames``, ``_game_diagnostics`` and ``_MirroredPartitionWriter`` over rows it simulated
(`tools/gen_seat_analysis_golden.py`) — with the same schema and every value bit-equal; the closed form of the pairing against the
two-queue loop, merge, the refusals."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import golden_util as gu  # noqa: E402
from seat_analysis_engine_stub import Engine as StubEngine  # noqa: E402

from farkle_ii_amd import seat_analysis as sa  # noqa: E402
from farkle_ii_amd.backend import make_overrides  # noqa: E402
from farkle_ii_amd.strategies import STRATEGY_DTYPE  # noqa: E402

CASES = gu.load("seat_analysis_vectors.json")["cases"]


def encode(table) -> dict:
    cols = {}
    for name in table.schema.names:
        cols[name] = [v.hex() if isinstance(v, float) and v == v else ("nan" if isinstance(v, float) else v)
                      for v in table.column(name).to_pylist()]
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def case_table(case):
    table = gu.strategies_from_tuples(case["strategies"], STRATEGY_DTYPE)
    return table, np.asarray(table["strategy_id"], dtype=np.int32)


def cell_overrides(cell):
    # fixture rows are (root, k, shuffle, game, max_rounds)
    return make_overrides((o[0], o[2], o[3], o[1], o[4]) for o in cell["overrides"]) if cell["overrides"] else None


def cell_result(eng, case, cell, begin=0, end=None, **kw):
    """(SeatCounts, MirroredPairs | None) of shuffles [begin, end) of a fixture cell."""
    table, ids = case_table(case)
    k, spb = cell["k"], cell["shuffles_per_batch"]
    res = eng.tournament_seat_counts(table, k, case["root_seed"], begin, cell["n_shuffles"] if end is None else end, shuffles_per_batch=spb,
                                     target_score=case["target_score"], max_rounds=case["max_rounds"], overrides=cell_overrides(cell),
                                     strategy_ids=ids, want_mirrored=k == 2, **kw)
    return sa.SeatCounts.from_engine(res, k, begin // spb), sa.MirroredPairs.from_engine(res, ids) if k == 2 else None


def check_case(case, results):
    """Every frame of the stage, built from ``results`` (one (counts, pairs) per cell), equals the reference's."""
    _, ids = case_table(case)
    root = case["root_seed"]
    by_k, population, counts_by_k = {}, {}, {}
    for cell, (counts, pairs) in zip(case["cells"], results):
        k = cell["k"]
        assert encode(sa.batch_counts_table(counts, ids, root)) == cell["batch_counts"], f"{case['name']} k={k} batch counts"
        by_k[k], population[k] = sa.within_k_frames(counts, ids, root)
        assert encode(by_k[k]) == cell["by_k"], f"{case['name']} k={k} by_k"
        assert encode(population[k]) == cell["population_by_k"], f"{case['name']} k={k} population"
        counts_by_k[k] = counts
        if k == 2:
            got = encode(sa.mirrored_frame(pairs, root))
            want = cell["mirrored"]
            assert [name for name, _ in got["schema"]] == list(want[0].keys())
            assert dict(got["schema"]) == {"root_seed": "int64", "k": "int16", "strategy_a": "int32", "strategy_b": "int32",
                                           "paired_mirrored_games": "int64", "games_attempted": "int64", "games_completed": "int64",
                                           "games_safety_limit": "int64", "unpaired_forward_games": "int64",
                                           "unpaired_reverse_games": "int64", "mean_p1_win_difference": "double"}
            assert [dict(zip(got["columns"], row)) for row in zip(*got["columns"].values())] == want, f"{case['name']} mirrored"
            # the shard rows summed over the batches: the six additive values per pair
            sums: dict = {}
            for _batch, a, b, *v in cell["mirrored_shards"]:
                t = sums.setdefault((a, b), [0] * 6)
                for j in range(6):
                    t[j] += v[j]
            assert {(int(a), int(b)): [int(x) for x in s] for (a, b), s in zip(pairs.ids, pairs.sums)} == sums
    ks = [cell["k"] for cell in case["cells"]]
    std, mix = sa.standardized_frames(by_k, population, ks, sa.declared_weights(ks))
    assert encode(std) == case["standardized_equal_k"] and encode(mix) == case["mixture_equal_k"], case["name"]
    if "declared_weights" in case:
        weights = {int(k): float.fromhex(w) for k, w in case["declared_weights"]}
        std, mix = sa.standardized_frames(by_k, population, ks, sa.declared_weights(ks, "declared-mapping", weights))
        assert encode(std) == case["standardized_declared"] and encode(mix) == case["mixture_declared"], case["name"]
    assert encode(sa.selfplay_frame(by_k)) == case["selfplay"], case["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_statement_reproduces_the_reference(case):
    eng = StubEngine()
    results = [cell_result(eng, case, cell) for cell in case["cells"]]
    for cell, (counts, _) in zip(case["cells"], results):
        games = counts.counts[:, :, 0, :].sum(axis=(0, 1))  # every game has one seat 1
        assert int(games[sa.SAFETY]) == cell["safety_limit_games"]
    check_case(case, results)


def test_fixture_covers_the_issue_cases():
    cells = [cell for case in CASES for cell in case["cells"]]
    assert {1, 2, 3, 4} <= {c["k"] for c in cells}
    assert any(c["absent_cells"] > 0 for c in cells)
    k2 = [c["coverage"] for c in cells if c["k"] == 2]
    assert len(k2) == 2
    for what in k2[0]:
        assert any(cov[what] for cov in k2), what
    assert any(len(c["mirrored_shards_3"]) and c["mirrored_shards_3"] == c["mirrored_shards"] for c in cells if c["k"] == 2)


def test_closed_form_equals_the_two_queue_loop():
    rng = np.random.default_rng(20240607)
    for _ in range(3000):
        n = int(rng.integers(0, 40))
        p_forward = rng.choice([0.1, 0.5, 0.9])
        o = np.where(rng.random(n) < 0.12, sa.SAFETY_GAME, np.where(rng.random(n) < p_forward, sa.FORWARD, sa.REVERSE))
        p1 = np.where(o == sa.SAFETY_GAME, 0, rng.integers(0, 2, n))
        assert sa.pair_closed_form(o, p1) == sa.pair_two_queue(o, p1)
    # a wrong rule (the LAST m games of the longer queue) would differ here
    assert sa.pair_two_queue([0, 0, 0, 1, 1], [1, 1, 0, 0, 0]) == (2, 2, 5, 0, 1, 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merge_over_batch_aligned_splits_is_one_range(case):
    eng = StubEngine()
    for cell in case["cells"]:
        spb, n = cell["shuffles_per_batch"], cell["n_shuffles"]
        whole_counts, whole_pairs = cell_result(eng, case, cell)
        cuts = [0] + list(range(spb, n, spb)) + [n]
        parts = [cell_result(eng, case, cell, a, b) for a, b in zip(cuts, cuts[1:])]
        for order in (parts, parts[::-1]):
            counts, pairs = order[0]
            for c, p in order[1:]:
                counts = counts.merge(c)
                pairs = pairs.merge(p) if pairs is not None else None
            assert counts.first_batch == 0 and np.array_equal(counts.counts, whole_counts.counts)
            if whole_pairs is not None:
                assert np.array_equal(pairs.ids, whole_pairs.ids) and np.array_equal(pairs.sums, whole_pairs.sums)


def test_duplicate_strategy_ids_are_refused():
    case = CASES[1]
    table, ids = case_table(case)
    ids = ids.copy()
    ids[1] = ids[0]
    with pytest.raises(ValueError, match="unique strategy IDs"):
        StubEngine().tournament_seat_counts(table, 2, 5, 0, 16, shuffles_per_batch=16, strategy_ids=ids, want_mirrored=True)
    with pytest.raises(ValueError, match="unique strategy IDs"):
        sa.batch_counts_table(sa.SeatCounts(2, 0, np.zeros((1, len(ids), 2, 3), np.int64)), ids, 5)


def test_declared_mapping_must_cover_every_k():
    assert sa.declared_weights([2, 3]) == {2: 0.5, 3: 0.5}
    assert sa.declared_weights([2, 3], "declared-mapping", {2: 0.25, 3: 0.75}) == {2: 0.25, 3: 0.75}
    with pytest.raises(ValueError, match="must cover every configured k"):
        sa.declared_weights([2, 3, 4], "declared-mapping", {2: 0.5, 3: 0.5})
    with pytest.raises(ValueError, match="must cover every configured k"):
        sa.declared_weights([2], "declared-mapping", {2: 0.5, 3: 0.5})


def test_null_rates_where_nothing_completed_or_paired():
    counts = sa.SeatCounts(2, 0, np.zeros((1, 2, 2, 3), np.int64))
    counts.counts[0, 0, 0] = (0, 0, 3)  # three safety-limit exposures, nothing completed
    counts.counts[0, 1, 1] = (1, 2, 1)
    by_k, _ = sa.within_k_frames(counts, [7, 5], 1)
    assert by_k.column("strategy").to_pylist() == [5, 7] and by_k.column("seat").to_pylist() == [2, 1]
    assert by_k.column("win_rate_given_completion").to_pylist() == [0.5, None]
    frame = sa.mirrored_frame(sa.MirroredPairs(np.array([[5, 7]]), np.array([[0, 0, 2, 1, 2, 0]])), 1)
    assert frame.column("mean_p1_win_difference").to_pylist() == [None] and frame.column("games_attempted").to_pylist() == [3]
