"""TEST INFRASTRUCTURE ONLY — write tests/golden/root_stability_frames_vectors.json by running the upstream Python reference in the
build container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The eight frames of the two-root stability stage that are no bootstrap family, by the reference's OWN functions over small synthetic
batch matrices saved in its ``_BATCH_MATRIX_DTYPE`` layout: ``_scope_estimates`` (the by-k frames of the three scopes and the
across-k frame), ``_rank_and_selection_stability`` (rank, top-N, control and shortlist frames), ``_matched_count_convergence`` and
``_half_drift``.  Every frame is recorded after ``_write_frame``'s strategy-id conversion as Arrow schema + columns, floats as
``float.hex`` (the encoding of tools/gen_root_stability_golden.py).  The ``np.dot`` columns of every across-k estimate the stage
makes — full, per matched count, per half — are recorded apart (``across_k``): they hold only on the machine that wrote them, and
the tests feed them back.

    python tools/gen_root_stability_frames_golden.py
"""
from __future__ import annotations

import sys
import tempfile
from math import ceil
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
sys.path.insert(0, str(HERE))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)
from gen_performance_bootstrap_golden import synthetic_matrix  # noqa: E402
from gen_root_stability_golden import encode, hexes  # noqa: E402

import pandas as pd  # noqa: E402
from farkle.analysis import root_stability as rs  # noqa: E402
from farkle.config import AppConfig  # noqa: E402

KINDS = {"wins": "raw_wins", "exposures": "raw_player_game_exposures", "completed": "raw_completed_player_game_exposures",
         "safety": "raw_safety_limit_player_game_exposures"}


def across_columns(frame) -> dict:
    ordered = frame.sort_values("strategy")
    return {"across_k_score": hexes(ordered["across_k_score"]), "across_k_mcse": hexes(ordered["across_k_mcse"])}


def case(name, matrices, roots, contribution, practical_by_k, delta_across_k, seed_stability, method, k_weights, controls, fractions,
         stage_batch_bytes=None):
    required_k = sorted({k for _, k in matrices})
    with tempfile.TemporaryDirectory() as folder:
        tmp = Path(folder)
        cfg = AppConfig()
        cfg.io.results_dir_prefix = tmp / "results"
        cfg.sim.n_players_list = list(required_k)
        cfg.screening.candidate_contribution_size = contribution
        cfg.screening.practical_delta_by_k = dict(practical_by_k)
        cfg.screening.delta_across_k = delta_across_k
        cfg.screening.controls = list(controls)
        cfg.robustness.delta_seed_stability = seed_stability
        cfg.robustness.matched_count_fractions = tuple(fractions)
        cfg.k_aggregation.method = method
        cfg.k_aggregation.k_weights = None if k_weights is None else dict(k_weights)
        if stage_batch_bytes is not None:
            cfg.resources.stage_batch_bytes = {**cfg.resources.stage_batch_bytes, "performance": int(stage_batch_bytes)}
        max_bytes = int(cfg.resources.stage_batch_bytes.get("performance", cfg.resources.stage_batch_bytes["analysis"]))
        cells = {}
        for (root, k), m in sorted(matrices.items()):
            path = tmp / f"root_{root}_{k}p_matrix.npy"
            np.save(path, m, allow_pickle=False)
            cells[(root, k)] = rs.RootBatchCell(root, k, tmp / f"root_{root}_{k}p.parquet", path)
        by_k_tables, across_by_scope = rs._scope_estimates(cfg, cells, roots, required_k)
        rank, top_n, control_frame, shortlist = rs._rank_and_selection_stability(cfg, roots, across_by_scope)
        convergence = rs._matched_count_convergence(cfg, cells, roots, required_k, across_by_scope)
        drift = rs._half_drift(cfg, cells, roots, required_k)
        # the np.dot columns of every across-k estimate the stage makes, by the same calls
        across_k = {"full": {scope: across_columns(frame) for scope, frame in across_by_scope.items()}}
        minimum = min(len(m) for m in matrices.values())
        for fraction in fractions:
            matched = min(minimum, max(1, ceil(minimum * fraction)))
            _, partial = rs._scope_estimates(cfg, cells, roots, required_k, maximum_batches=matched)
            across_k[f"matched_{matched}"] = {scope: across_columns(frame) for scope, frame in partial.items()}
        weights = rs._k_weights(cfg, required_k)
        for root in roots:
            for half in ("first_half", "second_half"):
                estimates = {}
                for k in required_k:
                    count = len(matrices[(root, k)])
                    bounds = (0, count // 2) if half == "first_half" else (count // 2, count)
                    estimates[k] = rs._estimate_matrix_cells(cfg, [cells[(root, k)]], k=k, estimate_scope=half, root_seed=root,
                                                             practical_delta=float(practical_by_k[k]), row_bounds=bounds)
                frame = rs._estimate_across_k(estimates, required_k=required_k, weights=weights, estimate_scope=half, root_seed=root,
                                              practical_delta=delta_across_k)
                across_k[f"{half}_{root}"] = {half: across_columns(frame)}
        across = pd.concat([across_by_scope[f"root_{root}"] for root in roots] + [across_by_scope["combined_roots"]], ignore_index=True)
    first = matrices[(roots[0], required_k[0])]
    return {"name": name, "roots": list(roots), "required_k": required_k, "candidate_contribution_size": contribution,
            "practical_delta_by_k": {str(k): v for k, v in practical_by_k.items()}, "delta_across_k": delta_across_k,
            "delta_seed_stability": seed_stability, "k_aggregation_method": method,
            "k_weights": None if k_weights is None else {str(k): v for k, v in k_weights.items()}, "controls": list(controls),
            "matched_count_fractions": list(fractions), "stage_batch_bytes": max_bytes,
            "strategies": np.asarray(first["strategy"][0], dtype=np.int64).tolist(),
            "matrices": [{"root": root, "k": k, "batch_ids": m["deterministic_batch_id"][:, 0].tolist(),
                          **{kind: m[field].tolist() for kind, field in KINDS.items()}} for (root, k), m in sorted(matrices.items())],
            "across_k": across_k,
            "frames": {**{f"performance_root_combination_{k}p": encode(by_k_tables[k]) for k in required_k},
                       "performance_root_combination_across_k": encode(across), "root_rank_stability": encode(rank),
                       "root_top_n_stability": encode(top_n), "root_control_movement": encode(control_frame),
                       "root_shortlist_changes": encode(shortlist), "root_matched_count_convergence": encode(convergence),
                       "root_half_drift": encode(drift)}}


def orders_differ(exposures) -> bool:
    """Whether sum(e * e) of one column added row by row differs from NumPy's sum of the vector."""
    e = np.asarray(exposures, dtype=np.float64)
    total = 0.0
    for v in (e * e).tolist():
        total += v
    return total != float(np.add.reduce(e * e))


def main():
    rng = np.random.default_rng(20261021)
    roots = (11, 23)
    ids9 = [7, 8, 12, 19, 20, 33, 41, 58, 60]
    main_case = {}
    for (root, k), batches in {(11, 2): 13, (23, 2): 8, (11, 3): 5, (23, 3): 6}.items():
        zero = [(1, 5), (3, 5), (2, 0)] if (root, k) == (11, 2) else [(4, 6)] if (root, k) == (23, 3) else ()
        m = synthetic_matrix(rng, root, k, range(batches), ids9, zero_cells=zero, scale=60)
        for field in m.dtype.names:  # strategies 19 and 20 hold the same counts in every cell: their rank goes by the id
            if field.startswith("raw_"):
                m[field][:, 4] = m[field][:, 3]
        main_case[(root, k)] = m
    c1 = case("k23_unequal", main_case, roots, 4, {2: 0.02, 3: 0.015}, 0.01, 0.03, "declared-mapping", {2: 0.6, 3: 0.4}, [8, 41, 8],
              (0.25, 0.5, 0.75, 1.0))
    short = {(root, k): synthetic_matrix(rng, root, k, range(b), [3, 4, 9, 10, 11], scale=60)
             for (root, k), b in {(11, 2): 3, (23, 2): 4, (11, 4): 3, (23, 4): 2}.items()}
    c2 = case("three_batches", short, roots, 7, {2: 0.02, 4: 0.02}, 0.01, 0.03, "equal-k", None, [], (0.25, 0.5, 0.75, 1.0))
    single = {(root, 2): synthetic_matrix(rng, root, 2, range(b), [5], scale=60) for root, b in ((3, 4), (4, 5))}
    c3 = case("one_strategy", single, (3, 4), 3, {2: 0.02}, 0.01, 0.03, "equal-k", None, [5], (0.5, 1.0))
    for seed in range(100):
        big_rng = np.random.default_rng([20261021, seed])
        big = {(root, k): synthetic_matrix(big_rng, root, k, range(12), list(range(1, 8)), scale=2 ** 30) for root in roots for k in (2, 3)}
        m = big[(11, 2)]
        if orders_differ(m["raw_player_game_exposures"][:, 6]):
            break
    else:
        raise SystemExit("no seed at which the two summation orders differ in the last column")
    c4 = case("chunks_3_3_1", big, roots, 3, {2: 0.02, 3: 0.02}, 0.01, 0.03, "equal-k", None, [2], (0.25, 0.5, 0.75, 1.0),
              stage_batch_bytes=57 * 12 * 3)
    path = gg.OUT / "root_stability_frames_vectors.json"
    gg._dump({"numpy": np.__version__, "cases": [c1, c2, c3, c4]}, open(path, "w"))
    print(path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
