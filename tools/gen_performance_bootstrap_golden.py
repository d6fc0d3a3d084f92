"""TEST INFRASTRUCTURE ONLY — write tests/golden/performance_bootstrap_vectors.json by running the upstream Python reference in the
build container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The performance stage's joint deterministic-batch bootstrap by the reference's OWN code over small synthetic batch matrices: the
matrices are saved in its ``_BATCH_MATRIX_DTYPE`` layout, ``_estimate_one_k_matrix`` + ``_across_k_estimates`` give the
complete-support strategies and their ``equal_k_score``, ``_BootstrapRangeWriter`` writes the replicate-score ``.npy`` of every range
and ``_reduce_bootstrap_ranges`` reduces them — with its stage plumbing (``run_partitioned_stage``, ``_bootstrap_identity``)
replaced by a loop that calls the writer per unit, as tools/gen_game_stats_golden.py replaces the game-stats stage's.  The frames are
recorded after ``_write_frame``'s strategy-id conversion (``canonical_strategy_ids``) as Arrow schema + columns; floats as
``float.hex``.

    python tools/gen_performance_bootstrap_golden.py            # the fixture
    python tools/gen_performance_bootstrap_golden.py --time     # the reference's range writer + reduction at the production shape
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
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pyarrow as pa  # noqa: E402
from farkle.analysis import performance as pf  # noqa: E402
from farkle.config import AppConfig  # noqa: E402
from farkle.utils.strategy_ids import canonical_strategy_ids  # noqa: E402


def synthetic_matrix(rng, root, k, batch_ids, strategies, zero_cells=(), scale=400, duplicate_pairs=False):
    """A canonical batch matrix with random counts (wins <= completed, attempted = completed + safety, losses = attempted - wins)."""
    B, S = len(batch_ids), len(strategies)
    m = np.zeros((B, S), dtype=pf._BATCH_MATRIX_DTYPE)
    completed = rng.integers(scale // 2, scale, size=(B, S))
    safety = rng.integers(0, 4, size=(B, S))
    wins = rng.integers(0, completed // k + 1)
    if duplicate_pairs:  # columns 2i and 2i + 1 hold the same counts: every replicate score is tied pairwise
        for a in (completed, safety, wins):
            a[:, 1::2] = a[:, 0:(S // 2) * 2:2]
    for b, s in zero_cells:
        completed[b, s] = safety[b, s] = wins[b, s] = 0
    m["root_seed"] = root
    m["deterministic_batch_id"] = np.asarray(batch_ids, dtype=np.int32)[:, None]
    m["strategy"] = np.asarray(strategies, dtype=np.int32)[None, :]
    m["raw_wins"], m["raw_completed_player_game_exposures"], m["raw_safety_limit_player_game_exposures"] = wins, completed, safety
    m["raw_player_game_exposures"] = completed + safety
    m["raw_losses"] = completed + safety - wins
    return m


def encode(frame) -> dict:
    frame = frame.copy()
    for column in ("strategy", "control_strategy"):  # _write_frame :1307-1314
        if column in frame:
            frame[column] = canonical_strategy_ids(frame[column], nullable=False, context=column)
    table = pa.Table.from_pandas(frame, preserve_index=False)
    cols = {name: [v.hex() if isinstance(v, float) else v for v in table.column(name).to_pylist()] for name in table.schema.names}
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def reference_bootstrap(tmp: Path, matrices: dict, replicates, delta, contribution, controls, range_size):
    """-> (strategies, observed equal_k_score, [(start, stop, scores)], bootstrap frame, contrasts frame, seconds of writer / reduce)."""
    cfg = AppConfig()
    cfg.io.results_dir_prefix = tmp / "results"
    cfg.screening.bootstrap_replicates = replicates
    cfg.screening.delta_across_k = delta
    cfg.screening.candidate_contribution_size = contribution
    cfg.screening.controls = list(controls)
    required_k = sorted(matrices)
    paths = []
    for k in required_k:
        path = tmp / f"{k}p_matrix.npy"
        np.save(path, matrices[k], allow_pickle=False)
        paths.append(path)
    budget = int(cfg.resources.stage_batch_bytes.get("performance", cfg.resources.stage_batch_bytes["analysis"]))
    estimates = {k: pf._estimate_one_k_matrix(p, k, cfg.screening.resolution_delta, 0.03, max_batch_bytes=budget)
                 for k, p in zip(required_k, paths)}
    across, strategies, _ = pf._across_k_estimates(estimates, required_k, delta)
    seconds = {"writer": 0.0}

    def run_units(*, root, unit_source, writer, **_):
        n = 0
        for unit in unit_source():
            out = Path(root) / "units" / unit.relative_output
            out.parent.mkdir(parents=True, exist_ok=True)
            t0 = time.perf_counter()
            writer(unit, out)
            seconds["writer"] += time.perf_counter() - t0
            n += 1
        return types.SimpleNamespace(required_units=n)

    orig = pf.run_partitioned_stage, pf._bootstrap_identity
    pf.run_partitioned_stage, pf._bootstrap_identity = run_units, lambda cfg, matrix_paths: None
    try:
        t0 = time.perf_counter()
        boot, contrasts = pf._reduce_bootstrap_ranges(cfg, matrix_paths=tuple(paths), across=across, strategies=strategies,
                                                      required_k=required_k, force=True,
                                                      guard=types.SimpleNamespace(check_before_schedule=lambda: None), range_size=range_size)
        seconds["total"] = time.perf_counter() - t0
    finally:
        pf.run_partitioned_stage, pf._bootstrap_identity = orig
    ranges = []
    for unit in pf._bootstrap_units(replicates, range_size):
        start, stop = unit.key
        ranges.append((int(start), int(stop), np.load(cfg.performance_bootstrap_ranges_dir() / "units" / unit.relative_output)))
    complete = across.loc[across["complete_support"]]
    observed = dict(zip(complete["strategy"].astype(int).tolist(), complete["equal_k_score"].astype(float).tolist()))
    return strategies, [observed[int(s)] for s in strategies], ranges, boot, contrasts, seconds


def case(name, root, matrices, replicates, delta, contribution, controls, range_size):
    with tempfile.TemporaryDirectory() as tmp:
        strategies, observed, ranges, boot, contrasts, _ = reference_bootstrap(Path(tmp), matrices, replicates, delta, contribution,
                                                                                controls, range_size)
    ties = sum(len(np.unique(row)) < len(row) for _, _, sc in ranges for row in sc)
    print(name, "strategies", len(strategies), "replicates with exact ties", ties, "of", replicates)
    return {"name": name, "root_seed": root, "replicates": replicates, "delta_across_k": delta, "candidate_contribution_size": contribution,
            "controls": list(controls), "range_size": range_size,
            "matrices": [{"k": k, "batch_ids": m["deterministic_batch_id"][:, 0].tolist(), "strategies": m["strategy"][0].tolist(),
                          "wins": m["raw_wins"].tolist(), "completed": m["raw_completed_player_game_exposures"].tolist(),
                          "safety": m["raw_safety_limit_player_game_exposures"].tolist()} for k, m in sorted(matrices.items())],
            "strategies": [int(s) for s in strategies], "equal_k_score": [v.hex() for v in observed],
            "ranges": [{"start": a, "stop": b, "scores": [[v.hex() for v in row] for row in sc.tolist()]} for a, b, sc in ranges],
            "bootstrap": encode(boot), "contrasts": encode(contrasts)}


def time_reference(replicates: int, repeats: int):
    """The reference's range writer + reduction at the production shape: 5 160 strategies, k in {2,3,4,5,6,8,10,12}, 100 batches each."""
    rng = np.random.default_rng(5)
    ids = np.arange(5160)
    matrices = {k: synthetic_matrix(rng, 7, k, range(100), ids, scale=43 * 2) for k in (2, 3, 4, 5, 6, 8, 10, 12)}
    for i in range(repeats):
        with tempfile.TemporaryDirectory() as tmp:
            *_, seconds = reference_bootstrap(Path(tmp), matrices, replicates, 0.03, 75, (0, 17), 50)
        print(json.dumps({"what": "reference range writer + reduction, one process", "S": 5160, "player_counts": 8, "batches_per_k": 100,
                          "replicates": replicates, "run": i, "writer_seconds": round(seconds["writer"], 3),
                          "total_seconds": round(seconds["total"], 3), "host_cpus": os.cpu_count()}), flush=True)


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
    main_case = {
        # 13 batches, batch 5 has a strategy without an exposure (12 eligible); one more strategy (id 500) than the other player counts
        2: synthetic_matrix(rng, 11, 2, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], ids96 + [500], zero_cells=[(5, 40)], scale=12),
        3: synthetic_matrix(rng, 11, 3, [0, 1, 2, 4, 5, 6, 7, 8, 9], ids96, scale=12),
        4: synthetic_matrix(rng, 11, 4, [0], ids96, scale=12),
    }
    ids24 = list(range(24))
    tied_case = {2: synthetic_matrix(rng, 5, 2, range(7), ids24, duplicate_pairs=True),
                 5: synthetic_matrix(rng, 5, 5, range(4), ids24, duplicate_pairs=True)}
    out = {"cases": [case("k234", 11, main_case, 64, 0.01, 10, (7, 151), 50),
                     case("tied_pairs", 5, tied_case, 64, 0.005, 75, (3,), 50)]}
    path = gg.OUT / "performance_bootstrap_vectors.json"
    gg._dump(out, open(path, "w"))
    print(path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
