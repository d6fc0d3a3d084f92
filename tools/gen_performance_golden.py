"""TEST INFRASTRUCTURE ONLY — write tests/golden/performance_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The performance stage's point estimates by the reference's OWN code over the golden subset of tests/performance_cases.py: the matrices
are saved in its ``_BATCH_MATRIX_DTYPE`` layout and ``_estimate_one_k_matrix`` reads them; ``_across_k_estimates`` runs over those
frames, once with a strategy of incomplete support and once without; ``_pareto_membership`` runs on the designed Pareto sets; and
``_build_screening_frame`` merges the complete-support frames with a bootstrap table, its artifact reader replaced by a plain Parquet
read of the files written here (the frames pass through ``_write_frame``'s strategy-id conversion and a Parquet round trip first, as in
the reference's stage).  Frames are recorded as Arrow schema + columns, floats as ``float.hex``.

    python tools/gen_performance_golden.py
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
sys.path.insert(0, str(HERE.parent / "tests"))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pandas as pd  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402
from farkle.analysis import performance as pf  # noqa: E402
from farkle.analysis import screening as sc  # noqa: E402
from farkle.config import AppConfig  # noqa: E402
from farkle.utils.strategy_ids import canonical_strategy_ids  # noqa: E402

import performance_cases as cases  # noqa: E402


def written(frame: pd.DataFrame) -> pa.Table:
    """The table ``_write_frame`` hands to the Parquet writer (:1307-1314)."""
    frame = frame.copy()
    for column in ("strategy", "control_strategy"):
        if column in frame:
            frame[column] = canonical_strategy_ids(frame[column], nullable=bool(frame[column].isna().any()), context=column)
    return pa.Table.from_pandas(frame, preserve_index=False)


def encode(table: pa.Table) -> dict:
    cols = {name: [v.hex() if isinstance(v, float) else v for v in table.column(name).to_pylist()] for name in table.schema.names}
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def reference_matrix(k: int, batch_ids, strategies, m: dict) -> np.ndarray:
    out = np.zeros(m["wins"].shape, dtype=pf._BATCH_MATRIX_DTYPE)
    out["root_seed"] = cases.GOLDEN_ROOT
    out["deterministic_batch_id"] = np.asarray(batch_ids, dtype=np.int32)[:, None]
    out["strategy"] = np.asarray(strategies, dtype=np.int32)[None, :]
    out["raw_wins"], out["raw_player_game_exposures"] = m["wins"], m["exposures"]
    out["raw_completed_player_game_exposures"], out["raw_safety_limit_player_game_exposures"] = m["completed"], m["safety"]
    out["raw_losses"] = m["exposures"] - m["wins"]
    return out


def run(tmp: Path, complete_only: bool) -> dict:
    settings = cases.GOLDEN_SCREENING
    cfg = AppConfig()
    cfg.io.results_dir_prefix = tmp / "results"
    cfg.sim.n_players_list = sorted(cases.GOLDEN_K)
    cfg.screening.resolution_delta = settings["resolution_delta"]
    cfg.screening.practical_delta_by_k = dict(settings["practical_delta_by_k"])
    cfg.screening.delta_across_k = settings["delta_across_k"]
    cfg.screening.candidate_contribution_size = settings["candidate_contribution_size"]
    cfg.screening.controls = list(settings["controls"])
    cfg.screening.mandatory_diagnostics = list(settings["mandatory_diagnostics"])
    required_k = sorted(cases.GOLDEN_K)
    budget = int(cfg.resources.stage_batch_bytes.get("performance", cfg.resources.stage_batch_bytes["analysis"]))
    estimates, by_k = {}, {}
    for k, (batch_ids, strategies, m) in sorted(cases.golden_matrices(complete_only).items()):
        path = tmp / f"{k}p_{int(complete_only)}.npy"
        np.save(path, reference_matrix(k, batch_ids, strategies, m), allow_pickle=False)
        estimates[k] = pf._estimate_one_k_matrix(path, k, settings["resolution_delta"], float(settings["practical_delta_by_k"][k]),
                                                 max_batch_bytes=budget)
        by_k[k] = written(estimates[k])
    across_frame, strategies, vectors = pf._across_k_estimates(estimates, required_k, settings["delta_across_k"])
    across = written(across_frame)
    out = {"by_k": {str(k): encode(t) for k, t in by_k.items()}, "across_k": encode(across),
           "complete_strategies": [int(s) for s in strategies]}
    if complete_only:
        files = {}
        for k, table in by_k.items():
            files[cfg.performance_by_k_path(k)] = table
        files[cfg.performance_across_k_path()] = across
        files[cfg.performance_bootstrap_path()] = pa.table(cases.golden_bootstrap_columns(strategies))
        for path, table in files.items():
            path.parent.mkdir(parents=True, exist_ok=True)
            pq.write_table(table, path)
        original = sc.read_parquet_artifact
        sc.read_parquet_artifact = lambda path, expected_sidecar=None: pq.read_table(path)
        try:
            frame = sc._build_screening_frame(cfg, required_k)
        finally:
            sc.read_parquet_artifact = original
        out["screening"] = encode(pa.Table.from_pandas(frame, preserve_index=False))
        out["payload"] = {"artifact": "descriptive_screening.parquet", "player_counts": required_k, "strategy_count": len(frame),
                          "pareto_count": int(frame["pareto_member"].sum()),
                          "maximin_leader": int(frame.loc[frame["maximin_leader"], "strategy"].iloc[0]),
                          "control_count": int(frame["declared_control"].sum()),
                          "mandatory_diagnostic_count": int(frame["mandatory_diagnostic"].sum())}
    return out


def main():
    out = {"numpy": np.__version__}
    with tempfile.TemporaryDirectory() as tmp:
        out["with_incomplete"] = run(Path(tmp), complete_only=False)
        out["complete"] = run(Path(tmp), complete_only=True)
    out["pareto"] = {}
    for kind, n, d in cases.GOLDEN_PARETO:
        values = cases.pareto_case(kind, n, d)
        member = pf._pareto_membership(values, np.arange(n, dtype=np.int64) * 3 + 1)
        out["pareto"][f"{kind}-n{n}-d{d}"] = "".join("1" if m else "0" for m in member.tolist())
    path = gg.OUT / "performance_vectors.json"
    gg._dump(out, open(path, "w"))
    print(path.stat().st_size, "bytes")
    for name in ("by_k", "across_k", "screening"):
        table = out["complete"][name] if name != "by_k" else out["complete"]["by_k"]["2"]
        print(name, table["schema"])
    print("across_k with an incomplete strategy", out["with_incomplete"]["across_k"]["schema"])


if __name__ == "__main__":
    main()
