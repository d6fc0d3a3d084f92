"""TEST INFRASTRUCTURE ONLY — what the performance-bootstrap tests share: the fixture's cases as ``BatchMatrix`` objects, table
encoding, synthetic matrices."""
from __future__ import annotations

import numpy as np

import golden_util as gu

from farkle_ii_amd import performance_bootstrap as pb

CASES = gu.load("performance_bootstrap_vectors.json")["cases"]


def case_matrices(case) -> dict:
    out = {}
    for m in case["matrices"]:
        completed, safety = np.asarray(m["completed"], np.int64), np.asarray(m["safety"], np.int64)
        out[int(m["k"])] = pb.BatchMatrix(int(case["root_seed"]), int(m["k"]), np.asarray(m["batch_ids"], np.int32),
                                         np.asarray(m["strategies"], np.int32), np.asarray(m["wins"], np.int64), completed + safety,
                                         completed, safety)
    return out


def case_scores(case) -> np.ndarray:
    """The reference's replicate scores of all ranges, ``[replicates][S]``."""
    return np.asarray([[float.fromhex(v) for v in row] for r in case["ranges"] for row in r["scores"]], dtype=np.float64)


def encode(table) -> dict:
    cols = {name: [v.hex() if isinstance(v, float) else v for v in table.column(name).to_pylist()] for name in table.schema.names}
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def synthetic(seed: int, S: int, batches: dict, low: int = 20, high: int = 90):
    """-> (ks, wins, exposures): random eligible matrices, ``batches`` = {k: B_k}; every exposure positive, wins <= exposures."""
    rng = np.random.default_rng(seed)
    ks = sorted(batches)
    exposures = [rng.integers(low, high, size=(batches[k], S), dtype=np.int64) for k in ks]
    wins = [rng.integers(0, e // k + 1, dtype=np.int64) for k, e in zip(ks, exposures)]
    return ks, wins, exposures


def assert_same(got: dict, want: dict, scores: bool = True) -> None:
    """Two results of ``performance_bootstrap`` (device, host statement): every output bit for bit."""
    if scores:
        assert got["scores"].dtype == np.float64 and got["scores"].shape == want["scores"].shape
        assert got["scores"].tobytes() == want["scores"].tobytes(), "replicate scores differ"
    for name in ("rank_sum", "rank_square_sum", "top_counts", "shortlist_counts"):
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), name
    for name in ("contrast_sum", "contrast_square_sum"):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
