"""TEST INFRASTRUCTURE ONLY — `tests/golden/root_stability_bootstrap_vectors.json` (tools/gen_root_stability_golden.py: the
reference's own two-root stability bootstrap families over synthetic batch matrices) decoded for the CPU and GPU tests."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from farkle_ii_amd import root_stability as rs
from farkle_ii_amd.performance_bootstrap import BatchMatrix

CASES = json.loads((Path(__file__).resolve().parent / "golden" / "root_stability_bootstrap_vectors.json").read_text())["cases"]


def by_name(name: str) -> dict:
    return next(c for c in CASES if c["name"] == name)


def floats(values) -> np.ndarray:
    return np.asarray([float.fromhex(v) for v in values], dtype=np.float64)


def case_matrices(case) -> dict:
    out = {}
    for m in case["matrices"]:
        exposures = np.asarray(m["exposures"], dtype=np.int64)  # (wins and exposures are all the stage reads: no safety-limit split)
        out[(m["root"], m["k"])] = BatchMatrix(m["root"], m["k"], np.asarray(m["batch_ids"], dtype=np.int32),
                                               np.asarray(case["strategies"], dtype=np.int32), np.asarray(m["wins"], dtype=np.int64),
                                               exposures, exposures, np.zeros_like(exposures))
    return out


def case_cells(case) -> rs.RootCells:
    return rs.check_cells(case_matrices(case), case["roots"], case["required_k"])


def case_weights(case) -> list:
    return floats(case["weights"]).tolist()


def case_across(case) -> dict:
    """The fixture's recorded ``np.dot`` columns, fed to ``scope_estimates`` (they hold only on the machine that wrote them): the scores
    are the discrepancy frame's across-k rows; the MCSE of the two roots is recorded apart, the combined scope's enters no output."""
    S = len(case["strategies"])
    frame = decode(case["root_discrepancies"] or case["root_discrepancies_before_joint"])["columns"]
    scopes = [f"root_{case['roots'][0]}", f"root_{case['roots'][1]}", "combined_roots"]
    out = {}
    for scope, column in zip(scopes, ("root_a_estimate", "root_b_estimate", "combined_estimate")):
        mcse = floats(expand(case["across_k"][scope]["across_k_mcse"])) if scope in case["across_k"] else np.full(S, np.nan)
        out[scope] = (floats(frame[column][-S:]), mcse)
    return out


def case_kwargs(case) -> dict:
    return dict(replicates=case["replicates"], candidate_contribution_size=case["candidate_contribution_size"],
                practical_delta_by_k={int(k): v for k, v in case["practical_delta_by_k"].items()}, delta_across_k=case["delta_across_k"],
                delta_seed_stability=case["delta_seed_stability"], joint_discrepancy_alpha=case["joint_discrepancy_alpha"],
                k_aggregation_method=case["k_aggregation_method"],
                declared_k_weights=None if case["k_weights"] is None else {int(k): v for k, v in case["k_weights"].items()})


def case_joint(case, cells=None):
    """(discrepancy frame before the joint columns, JointInputs) by the host chain with the fixture's across-k columns fed in."""
    cells = cells or case_cells(case)
    kw = case_kwargs(case)
    estimates = rs.scope_estimates(cells, case_weights(case), kw["practical_delta_by_k"], kw["delta_across_k"], across_k=case_across(case))
    frame = rs.discrepancies(estimates, cells, kw["delta_seed_stability"])
    return estimates, frame, rs.joint_inputs(frame, len(cells.required_k), len(cells.strategies))


def case_ranges(case):
    """[(start, stop, membership uint8 [n][2][S], maxima float64 [n])] of the reference's range files."""
    S = len(case["strategies"])
    out = []
    for r in case["ranges"]:
        n = r["stop"] - r["start"]
        member = np.zeros((n, 2, S), dtype=np.uint8)
        for i, rep in enumerate(r["top_n_members"]):
            for root_index, columns in enumerate(rep):
                member[i, root_index, columns] = 1
        out.append((r["start"], r["stop"], member, floats(r["maxima"])))
    return out


def expand(v) -> list:
    """A fixture column: a list, ``{"const": v, "n": rows}`` or ``{"dict": distinct, "idx": positions}``."""
    if isinstance(v, dict):
        return [v["const"]] * v["n"] if "const" in v else [v["dict"][i] for i in v["idx"]]
    return v


def decode(frame: dict) -> dict:
    """An encoded fixture frame -> {"schema": [[name, type]], "columns": {name: list}} with floats still as ``float.hex``."""
    return {"schema": frame["schema"], "columns": {name: expand(v) for name, v in frame["columns"].items()}}


def encode(table) -> dict:
    """An Arrow table in the decoded fixture form."""
    cols = {name: [v.hex() if isinstance(v, float) else v for v in table.column(name).to_pylist()] for name in table.schema.names}
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def synthetic(seed: int, S: int, batches_a: dict, batches_b: dict | None = None, low: int = 20, high: int = 90):
    """-> (ks, wins, exposures) of the 2 x n_k cells in (root, k) order: random eligible matrices, ``batches_x`` = {k: B} of root x;
    every exposure positive, wins <= exposures."""
    rng = np.random.default_rng(seed)
    ks = sorted(batches_a)
    batches_b = batches_a if batches_b is None else batches_b
    assert sorted(batches_b) == ks
    exposures = [rng.integers(low, high, size=(b[k], S), dtype=np.int64) for b in (batches_a, batches_b) for k in ks]
    wins = [rng.integers(0, e // k + 1, dtype=np.int64) for k, e in zip(ks + ks, exposures)]
    return ks, wins, exposures


def synthetic_joint(seed: int, n_k: int, S: int, odd: bool = True) -> dict:
    """observed / expected of the joint family; ``odd``: about a quarter of the expected entries are NaN, 0, -0.0, negative or inf
    (no estimand, or one whose value is 0)."""
    rng = np.random.default_rng(seed)
    out = {"observed": rng.normal(0.0, 0.02, size=(n_k, S)), "expected": rng.uniform(0.005, 0.05, size=(n_k, S)),
           "observed_across": rng.normal(0.0, 0.01, size=S), "expected_across": rng.uniform(0.002, 0.02, size=S)}
    if odd:
        for name in ("expected", "expected_across"):
            flat = out[name].reshape(-1)
            pick = rng.random(flat.size) < 0.25
            flat[pick] = rng.choice([np.nan, 0.0, -0.0, -0.01, np.inf], size=int(pick.sum()))
    return out


def assert_same(got: dict, want: dict) -> None:
    """Two results of ``root_stability_bootstrap`` (device, host statement): every output as bytes."""
    assert got["top_counts"].dtype == np.int64 and got["top_counts"].shape == want["top_counts"].shape and want["top_counts"].size
    assert got["top_counts"].tobytes() == want["top_counts"].tobytes(), "top-N inclusion counts differ"
    for name, dtype in (("maxima", np.float64), ("membership", np.uint8)):
        assert (got[name] is None) == (want[name] is None), name
        if want[name] is not None:
            assert got[name].dtype == dtype and got[name].shape == want[name].shape
            assert got[name].tobytes() == want[name].tobytes(), f"{name} differ"
