"""TEST INFRASTRUCTURE ONLY — write tests/golden/root_stability_bootstrap_vectors.json by running the upstream Python reference in the
build container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The two-root stability stage's bootstrap families by the reference's OWN code over small synthetic batch matrices: the matrices of
two roots x all player counts are saved in its ``_BATCH_MATRIX_DTYPE`` layout, ``_scope_estimates`` + ``_discrepancies`` give the
discrepancy frame, ``_joint_discrepancy_bootstrap`` (``_JointDiscrepancyRangeWriter``) and ``_root_bootstrap_top_n_inclusion``
(``_RootTopNRangeWriter``) write every range ``.npy`` and reduce them — with the stage plumbing replaced: ``run_partitioned_stage`` by a
loop that calls the writer per unit, ``_root_bootstrap_identity`` and the two ``cfg.root_stability_*_ranges_dir`` methods by stand-ins
(the stage is not in a bare ``AppConfig``'s layout).  Frames are recorded after ``_write_frame``'s strategy-id conversion as Arrow schema
+ columns; floats as ``float.hex``; a column of one repeated value as ``{"const": v, "n": rows}``, a string column as dictionary +
indices; membership as the sorted top-N column lists.

    python tools/gen_root_stability_golden.py            # the fixture
    python tools/gen_root_stability_golden.py --time     # both reference writers + reductions at the production shape
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
sys.path.insert(0, str(HERE))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)
from gen_performance_bootstrap_golden import synthetic_matrix  # noqa: E402

import pyarrow as pa  # noqa: E402
from farkle.analysis import root_stability as rs  # noqa: E402
from farkle.config import AppConfig  # noqa: E402
from farkle.utils.strategy_ids import canonical_strategy_ids  # noqa: E402


def hexes(values) -> list:
    return [float(v).hex() for v in np.asarray(values, dtype=np.float64).reshape(-1)]


def compact(values: list):
    """A column as a list, ``{"const": v, "n": rows}`` or ``{"dict": distinct, "idx": positions}``, whichever is shortest to read."""
    distinct = list(dict.fromkeys(values))
    if len(distinct) == 1 and len(values) > 1:
        return {"const": distinct[0], "n": len(values)}
    if len(values) > 8 and len(distinct) <= len(values) // 2:
        return {"dict": distinct, "idx": [distinct.index(v) for v in values]}
    return values


def encode(frame) -> dict:
    frame = frame.copy()
    if "strategy" in frame:  # _write_frame :1646-1652
        frame["strategy"] = canonical_strategy_ids(frame["strategy"], nullable=bool(frame["strategy"].isna().any()), context="strategy")
    table = pa.Table.from_pandas(frame, preserve_index=False)
    cols = {}
    for name in table.schema.names:
        cols[name] = compact([v.hex() if isinstance(v, float) else v for v in table.column(name).to_pylist()])
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "rows": table.num_rows, "columns": cols}


def reference_stage(tmp: Path, matrices: dict, roots, replicates, contribution, practical_by_k, delta_across_k, seed_stability, alpha,
                    method, k_weights, estimates_only=False):
    """``matrices``: {(root, k): canonical matrix}.  -> dict of everything the stage's two families consume and produce."""
    cfg = AppConfig()
    cfg.io.results_dir_prefix = tmp / "results"
    required_k = sorted({k for _, k in matrices})
    cfg.sim.n_players_list = list(required_k)
    cfg.screening.bootstrap_replicates = replicates
    cfg.screening.candidate_contribution_size = contribution
    cfg.screening.practical_delta_by_k = dict(practical_by_k)
    cfg.screening.delta_across_k = delta_across_k
    cfg.robustness.delta_seed_stability = seed_stability
    cfg.robustness.joint_discrepancy_alpha = alpha
    cfg.k_aggregation.method = method
    cfg.k_aggregation.k_weights = None if k_weights is None else dict(k_weights)
    cells = {}
    for (root, k), m in sorted(matrices.items()):
        path = tmp / f"root_{root}_{k}p_matrix.npy"
        np.save(path, m, allow_pickle=False)
        cells[(root, k)] = rs.RootBatchCell(root, k, tmp / f"root_{root}_{k}p.parquet", path)
    seconds = {"top_n_writer": 0.0, "joint_writer": 0.0}
    dirs = {"top_n": tmp / "top_n_ranges", "joint": tmp / "joint_ranges"}

    def run_units(*, root, unit_source, writer, **_):
        family = "top_n_writer" if isinstance(writer, rs._RootTopNRangeWriter) else "joint_writer"
        n = 0
        for unit in unit_source():
            out = Path(root) / "units" / unit.relative_output
            out.parent.mkdir(parents=True, exist_ok=True)
            t0 = time.perf_counter()
            writer(unit, out)
            seconds[family] += time.perf_counter() - t0
            n += 1
        return types.SimpleNamespace(required_units=n)

    cls = type(cfg)
    orig = (rs.run_partitioned_stage, rs._root_bootstrap_identity, cls.root_stability_top_n_ranges_dir, cls.root_stability_joint_ranges_dir)
    rs.run_partitioned_stage, rs._root_bootstrap_identity = run_units, lambda cfg, cells, roots, family: None
    cls.root_stability_top_n_ranges_dir = lambda self: dirs["top_n"]
    cls.root_stability_joint_ranges_dir = lambda self: dirs["joint"]
    guard = types.SimpleNamespace(check_before_schedule=lambda **_: None)
    try:
        weights = rs._k_weights(cfg, required_k)
        t0 = time.perf_counter()
        by_k_tables, across_by_scope = rs._scope_estimates(cfg, cells, roots, required_k)
        discrepancies = rs._discrepancies(cfg, roots, by_k_tables, across_by_scope)
        seconds["estimates"] = time.perf_counter() - t0
        out = {"cfg": cfg, "required_k": required_k, "weights": [weights[k] for k in required_k], "by_k_tables": by_k_tables,
               "across_by_scope": across_by_scope, "discrepancies": discrepancies, "seconds": seconds}
        if estimates_only:
            return out
        t0 = time.perf_counter()
        try:
            enriched, summary = rs._joint_discrepancy_bootstrap(cfg, cells, roots, required_k, discrepancies, force=True, guard=guard)
        except TypeError as exc:
            # every standardized_discrepancy None: the column is of dtype object and the reference's own reduction fails at
            # `.abs()` (:1399) AFTER its writer has written every range; the ranges are recorded, the frames cannot be
            enriched, summary, out["reduction_error"] = None, None, f"{type(exc).__name__}: {exc}"
        seconds["joint_total"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        inclusion = rs._root_bootstrap_top_n_inclusion(cfg, cells, roots, required_k, force=True, guard=guard)
        seconds["top_n_total"] = time.perf_counter() - t0
    finally:
        rs.run_partitioned_stage, rs._root_bootstrap_identity, cls.root_stability_top_n_ranges_dir, cls.root_stability_joint_ranges_dir = orig
    ranges = []
    for unit in rs._root_bootstrap_units(replicates):
        start, stop = unit.key
        ranges.append((int(start), int(stop), np.load(dirs["top_n"] / "units" / unit.relative_output),
                       np.load(dirs["joint"] / "units" / unit.relative_output)))
    out.update(enriched=enriched, summary=summary, inclusion=inclusion, ranges=ranges)
    return out


def case(name, matrices, roots, replicates, contribution, practical_by_k, delta_across_k, seed_stability, alpha, method, k_weights):
    with tempfile.TemporaryDirectory() as tmp:
        res = reference_stage(Path(tmp), matrices, roots, replicates, contribution, practical_by_k, delta_across_k, seed_stability, alpha,
                              method, k_weights)
    required_k = res["required_k"]
    scopes = [f"root_{roots[0]}", f"root_{roots[1]}", "combined_roots"]
    strategies = np.asarray(matrices[(roots[0], required_k[0])]["strategy"][0], dtype=np.int64)
    S = len(strategies)
    top_n = min(contribution, S)
    by_k = {}
    for k in required_k:
        table = res["by_k_tables"][k]
        by_k[str(k)] = {scope: {"batch_mcse": compact(hexes(table.loc[table["estimate_scope"].eq(scope)].sort_values("strategy")["batch_mcse"]))}
                        for scope in scopes[:2]}  # (the combined scope's MCSE enters no output of the two families)
    # (the across-k SCORES of the three scopes are the frame's across_k rows: root_a_estimate, root_b_estimate, combined_estimate)
    across = {scope: {"across_k_mcse": compact(hexes(res["across_by_scope"][scope].sort_values("strategy")["across_k_mcse"]))} for scope in scopes[:2]}
    disc = res["discrepancies"]
    expected_mcse = disc["expected_mcse"].to_numpy(dtype=float)
    maxima = np.concatenate([m for *_, m in res["ranges"]])
    members = np.concatenate([t for _, _, t, _ in res["ranges"]])
    assert members.shape == (replicates, 2, S) and maxima.shape == (replicates,)
    assert np.all(members.sum(axis=2) == top_n)
    split_pairs = int(np.sum(members[:, :, 0:(S // 2) * 2:2] != members[:, :, 1::2][:, :, :S // 2], axis=2).sum())
    print(name, "S", S, "valid estimands", int(np.sum(expected_mcse > 0.0)), "of", len(expected_mcse), "distinct maxima",
          len(np.unique(maxima)), "of", replicates, "columns 2i / 2i+1 with different membership (all rows)", split_pairs,
          "reduction", res.get("reduction_error", "ok"))
    out = {"name": name, "roots": list(roots), "required_k": required_k, "replicates": replicates, "candidate_contribution_size": contribution,
           "practical_delta_by_k": {str(k): v for k, v in practical_by_k.items()}, "delta_across_k": delta_across_k,
           "delta_seed_stability": seed_stability, "joint_discrepancy_alpha": alpha, "k_aggregation_method": method,
           "k_weights": None if k_weights is None else {str(k): v for k, v in k_weights.items()}, "weights": hexes(res["weights"]),
           "strategies": strategies.tolist(), "top_n": top_n,
           "matrices": [{"root": root, "k": k, "batch_ids": m["deterministic_batch_id"][:, 0].tolist(), "wins": m["raw_wins"].tolist(),
                         "exposures": m["raw_player_game_exposures"].tolist()} for (root, k), m in sorted(matrices.items())],
           "by_k": by_k, "across_k": across,
           "ranges": [{"start": a, "stop": b, "top_n_members": [[np.flatnonzero(row).tolist() for row in rep] for rep in t],
                       "maxima": hexes(m)} for a, b, t, m in res["ranges"]],
           "root_bootstrap_top_n_inclusion": encode(res["inclusion"]),
           "root_discrepancies_before_joint": encode(res["discrepancies"]) if res["enriched"] is None else None,
           "root_discrepancies": None if res["enriched"] is None else encode(res["enriched"]),
           "root_joint_discrepancy": None if res["summary"] is None else encode(res["summary"]),
           "reference_reduction_error": res.get("reduction_error")}
    return out, res, {"expected_mcse": expected_mcse, "maxima": maxima, "split_pairs": split_pairs, "members": members}


def production_matrices():
    rng = np.random.default_rng(5)
    ids = np.arange(5160)
    return {(root, k): synthetic_matrix(rng, root, k, range(100), ids, scale=43 * 2) for root in (7, 19) for k in (2, 3, 4, 5, 6, 8, 10, 12)}


def time_reference(replicates: int, repeats: int):
    """Both reference writers + reductions at the production shape: 2 roots, 5 160 strategies, k in {2,3,4,5,6,8,10,12}, 100 batches."""
    matrices = production_matrices()
    ks = sorted({k for _, k in matrices})
    for i in range(repeats):
        with tempfile.TemporaryDirectory() as tmp:
            res = reference_stage(Path(tmp), matrices, (7, 19), replicates, 75, {k: 0.03 for k in ks}, 0.03, 0.03, 0.05, "equal-k", None)
        print(json.dumps({"what": "reference root-stability range writers + reductions, one process", "S": 5160, "roots": 2, "player_counts": 8,
                          "batches_per_cell": 100, "replicates": replicates, "run": i,
                          **{f"{name}_seconds": round(v, 3) for name, v in res["seconds"].items()}, "host_cpus": os.cpu_count()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    if args.time:
        return time_reference(args.replicates, args.repeats)
    rng = np.random.default_rng(20261016)
    ids96 = [3 * i + 1 for i in range(96)]
    roots = (11, 23)
    gap = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    main_case = {}
    for root in roots:
        main_case[(root, 2)] = synthetic_matrix(rng, root, 2, range(13), ids96, zero_cells=[(5, 40)] if root == 11 else (), scale=12)
        main_case[(root, 3)] = synthetic_matrix(rng, root, 3, gap, ids96, scale=12)
        main_case[(root, 4)] = synthetic_matrix(rng, root, 4, [0, 1], ids96, scale=12)
    c1, _, p1 = case("k234", main_case, roots, 64, 10, {2: 0.02, 3: 0.02, 4: 0.02}, 0.01, 0.03, 0.05, "declared-mapping",
                     {2: 0.5, 3: 0.3, 4: 0.2})
    assert np.all(p1["expected_mcse"] > 0.0) and len(p1["expected_mcse"]) == 4 * 96 and len(np.unique(p1["maxima"])) == 64
    tied = {}
    for root in roots:
        tied[(root, 2)] = synthetic_matrix(rng, root, 2, range(7), ids96, duplicate_pairs=True)
        tied[(root, 3)] = synthetic_matrix(rng, root, 3, range(4), ids96, duplicate_pairs=True)
        tied[(root, 4)] = synthetic_matrix(rng, root, 4, [3], ids96, duplicate_pairs=True)
    c2, _, p2 = case("tied_pairs_one_batch", tied, roots, 64, 9, {2: 0.02, 3: 0.02, 4: 0.02}, 0.01, 0.03, 0.05, "equal-k", None)
    e2 = p2["expected_mcse"].reshape(4, 96)
    assert np.all(e2[:2] > 0.0) and np.all(np.isnan(e2[2:])), "k = 2, 3 valid; k = 4 and across-k invalid"
    m2 = p2["members"]
    per_row = np.sum(m2[:, :, 0::2] != m2[:, :, 1::2], axis=2)
    assert np.all(per_row == 1), "odd top_n over tied pairs: exactly one split pair per (replicate, root)"
    assert np.all(m2[:, :, 0::2] >= m2[:, :, 1::2]), "the lower id of a tied pair wins"
    ids8 = list(range(5, 13))
    invalid = {(root, k): synthetic_matrix(rng, root, k, [2], ids8) for root in (3, 4) for k in (2, 5)}
    c3, _, p3 = case("all_invalid", invalid, (3, 4), 64, 5, {2: 0.02, 5: 0.02}, 0.01, 0.03, 0.05, "equal-k", None)
    assert np.all(p3["maxima"] == 0.0) and not np.any(p3["expected_mcse"] > 0.0)
    assert c3["reference_reduction_error"] and c3["root_discrepancies"] is None  # (the reference cannot reduce this case: see reference_stage)
    path = gg.OUT / "root_stability_bootstrap_vectors.json"
    gg._dump({"cases": [c1, c2, c3]}, open(path, "w"))
    print(path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
