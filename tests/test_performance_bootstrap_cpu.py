"""The performance stage's joint batch bootstrap on the CPU: the NumPy host statement and the frame builders against
`tests/golden/performance_bootstrap_vectors.json` — the reference's OWN ``_BootstrapRangeWriter`` and ``_reduce_bootstrap_ranges``
over synthetic batch matrices (`tools/gen_performance_bootstrap_golden.py`) — bit for bit; the restated bounded draw against
``Generator.integers``; the matrix layout, its conservation checks, the projection and the error cases."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import performance_bootstrap_cases as pc  # noqa: E402
from performance_bootstrap_engine_stub import Engine as StubEngine  # noqa: E402

from farkle_ii_amd import performance_bootstrap as pb  # noqa: E402
from farkle_ii_amd.backend import SEAT_STAT_NAMES  # noqa: E402
from farkle_ii_amd.random import RandomPurpose, coordinate_seed_sequence  # noqa: E402


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c["name"])
def test_host_statement_matches_reference(case):
    matrices = pc.case_matrices(case)
    required = sorted(matrices)
    projection = pb.project(matrices, required)
    assert projection.strategies.tolist() == case["strategies"]
    want = pc.case_scores(case)
    for r in case["ranges"]:  # the range writer's payload, range by range
        got = pb.host_scores(case["root_seed"], projection.required_k, projection.wins, projection.exposures, r["start"], r["stop"])
        assert got.tobytes() == want[r["start"]:r["stop"]].tobytes()
    observed = pb.equal_k_scores(matrices, required, projection.strategies)
    assert [v.hex() for v in observed.tolist()] == case["equal_k_score"]
    for range_size in (None, case["range_size"], 7):  # any split of the replicates: the same frames
        boot, contrasts = pb.performance_bootstrap_tables(StubEngine(), matrices, required, case["replicates"],
                                                          case["candidate_contribution_size"], case["delta_across_k"], case["controls"],
                                                          range_size=range_size)
        assert pc.encode(boot) == case["bootstrap"]
        assert pc.encode(contrasts) == case["contrasts"]


def test_tied_scores_rank_by_column():
    case = next(c for c in pc.CASES if c["name"] == "tied_pairs")
    scores = pc.case_scores(case)
    assert all(np.array_equal(row[0::2], row[1::2]) for row in scores)  # every pair of columns is tied in every replicate
    ranks = case["bootstrap"]["columns"]["bootstrap_rank_mean"]
    assert all(float.fromhex(ranks[i + 1]) == float.fromhex(ranks[i]) + 1.0 for i in range(0, len(ranks), 2))


@pytest.mark.parametrize("bound", [1, 2, 100, 4300, 2 ** 31 + 1])
def test_bounded_draws_match_numpy(bound):
    for replicate in range(6):
        seq = lambda: coordinate_seed_sequence(RandomPurpose.BOOTSTRAP, root_seed=9, k=3, replicate_index=replicate)  # noqa: E731
        want = np.random.Generator(np.random.PCG64DXSM(seq())).integers(0, bound, size=301)
        got = pb.bounded_draws(np.random.PCG64DXSM(seq()), bound, 301)
        assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        pb.bounded_draws(np.random.PCG64DXSM(1), 2 ** 32, 1)


def test_matrix_round_trip_and_conservation(tmp_path):
    case = pc.CASES[0]
    m = pc.case_matrices(case)[2]
    arr = m.to_reference_array()
    assert arr.dtype == pb.BATCH_MATRIX_DTYPE and arr.dtype.itemsize == 56 and arr.shape == m.wins.shape
    back = pb.BatchMatrix.from_reference_array(arr, 2)
    for name in ("batch_ids", "strategies", "wins", "exposures", "completed", "safety"):
        assert np.array_equal(getattr(back, name), getattr(m, name)), name
    m.save(tmp_path / "by_k" / "2p" / "performance_batch_matrix.npy")
    loaded = np.load(tmp_path / "by_k" / "2p" / "performance_batch_matrix.npy")
    assert loaded.tobytes() == arr.tobytes()
    for field, message in (("raw_losses", "loss conservation"), ("raw_completed_player_game_exposures", "exposure conservation")):
        bad = arr.copy()
        bad[field][1, 2] += 1
        with pytest.raises(ValueError, match=message):
            pb.BatchMatrix.from_reference_array(bad, 2)
    bad = arr.copy()
    bad["raw_wins"][0, 0] = bad["raw_completed_player_game_exposures"][0, 0] + 1
    with pytest.raises(ValueError, match="impossible"):
        pb.BatchMatrix.from_reference_array(bad, 2)
    bad = arr.copy()
    bad["strategy"][:, 1] = bad["strategy"][:, 0]
    with pytest.raises(ValueError, match="strictly increasing"):
        pb.BatchMatrix.from_reference_array(bad, 2)
    with pytest.raises(ValueError, match="not a canonical"):
        pb.BatchMatrix.from_reference_array(arr.astype([(n, "<i8") for n in arr.dtype.names]), 2)


def test_matrix_from_seat_stats():
    col = {name: i for i, name in enumerate(SEAT_STAT_NAMES)}
    rng = np.random.default_rng(3)
    st = np.zeros((3, 5, len(SEAT_STAT_NAMES)), np.int64)
    st[:, :, col["completed_exposures"]] = rng.integers(5, 9, size=(3, 5))
    st[:, :, col["safety_limit_exposures"]] = rng.integers(0, 2, size=(3, 5))
    st[:, :, col["exposures"]] = st[:, :, col["completed_exposures"]] + st[:, :, col["safety_limit_exposures"]]
    st[:, :, col["wins"]] = rng.integers(0, 5, size=(3, 5))
    st[:, 3] = 0  # a strategy that never sits is no column of the matrix
    ids = [40, 10, 30, 20, 50]
    m = pb.BatchMatrix.from_seat_stats(st, ids, 7, 2, [2, 0, 1])
    assert m.strategies.tolist() == [10, 30, 40, 50] and m.batch_ids.tolist() == [0, 1, 2]
    assert np.array_equal(m.wins[0], st[1][[1, 2, 0, 4], col["wins"]])  # batch 0 is the second block, columns by ascending id
    m.to_reference_array()
    st[1, 0] = 0  # ... one that misses a single batch has no row there: the reference's matrix writer refuses the table
    with pytest.raises(ValueError, match="rectangular"):
        pb.BatchMatrix.from_seat_stats(st, ids, 7, 2, [2, 0, 1])


def test_projection():
    case = pc.CASES[0]
    matrices = pc.case_matrices(case)
    p = pb.project(matrices, [2, 3, 4])
    assert 500 not in p.strategies.tolist() and len(p.strategies) == 96  # id 500 only has a 2-player column
    assert [len(w) for w in p.wins] == [12, 9, 1] and p.eligible[0].tolist() == [b for b in range(13) if b != 5]
    assert all((e > 0).all() for e in p.exposures)
    with pytest.raises(ValueError, match="lacks complete configured strategy support"):
        pb.project(matrices, [2, 3], strategies=[1, 4, 500])
    none = pc.case_matrices(case)
    none[4].exposures[0, 3] = none[4].completed[0, 3] = none[4].wins[0, 3] = 0
    with pytest.raises(ValueError, match="no positive exposure support"):
        pb.project(none, [2, 3, 4])
    with pytest.raises(ValueError, match="no positive-exposure batch vectors"):
        pb.project(none, [2, 3, 4], strategies=p.strategies)
    other = pc.case_matrices(case)
    other[3].root_seed = 12
    with pytest.raises(ValueError, match="disagree on root"):
        pb.project(other, [2, 3, 4])


def test_error_cases():
    case = pc.CASES[0]
    matrices = pc.case_matrices(case)
    args = (StubEngine(), matrices, [2, 3, 4], 8, 10)
    with pytest.raises(ValueError, match="delta_across_k is required"):
        pb.performance_bootstrap_tables(*args, None, [])
    with pytest.raises(ValueError, match="declared controls lack complete k support: \\[500\\]"):
        pb.performance_bootstrap_tables(*args, 0.01, [7, 500])
    ks, wins, exposures = pc.synthetic(1, 6, {2: 3})
    exposures[0][:, 2] = 0
    with pytest.raises(ValueError, match="zero complete-support exposure"):
        pb.host_bootstrap(1, ks, wins, exposures, 0, 2, 1, 0.0)
    boot, contrasts = pb.performance_bootstrap_tables(*args, 0.01, [])  # no controls: an empty frame with the full schema
    assert contrasts.num_rows == 0 and contrasts.schema.equals(pb.contrast_schema()) and boot.num_rows == 96
    assert boot.column("top_n_size").to_pylist() == [10] * 96


def test_write_bootstrap_range(tmp_path):
    case = pc.CASES[0]
    matrices = pc.case_matrices(case)
    paths = []
    for k in (2, 3, 4):
        paths.append(tmp_path / f"{k}p" / "performance_batch_matrix.npy")
        matrices[k].save(paths[-1])
    r = case["ranges"][1]
    out = tmp_path / "replicates.npy"
    pb.write_bootstrap_range(StubEngine(), paths, [2, 3, 4], case["strategies"], case["root_seed"], r["start"], r["stop"], out)
    got = np.load(out)
    assert got.dtype == np.dtype("<f8") and got.tobytes() == pc.case_scores(case)[r["start"]:r["stop"]].tobytes()
