"""TEST INFRASTRUCTURE ONLY — write tests/golden/game_stats_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The game-stats stage of the reference by its OWN code over rows it simulated: ``_play_one_shuffle(collect_rows=True)`` ->
``simulation_rows_to_table`` (optionally padded to twelve seats with null ``P#_strategy`` / ``P#_score`` columns, as the combine
stage pads them) -> one parquet file per k -> ``_compute_k_game_stats`` itself, with ``_write_scoped_game_stats`` /
``write_stage_done`` replaced to capture the frame (as the reference's tests/unit/analysis/test_game_stats_branches.py:261-330
calls it) -> ``pa.Table.from_pandas(frame, preserve_index=False)``; and ``_rare_event_flags`` over the per-k files, of whose output
the summary rows (``summary_level`` "strategy" / "n_players") are kept.  Floats are recorded as ``float.hex``.

    python tools/gen_game_stats_golden.py
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pyarrow as pa  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402
from farkle.analysis import game_stats as gs  # noqa: E402
from farkle.config import AppConfig  # noqa: E402
from farkle.simulation.simulation import simulation_rows_to_table  # noqa: E402


def simulate(strategies, k, root, n_sh, target, max_rounds, overrides, pad_to):
    gp = gg.GameProfile(default_target_score=target, default_max_rounds=max_rounds,
                        tournament_max_rounds_overrides=tuple(gg.TournamentMaxRoundsOverride(*o) for o in overrides))
    cfg = gg.rt.TournamentConfig(n_players=k, num_shuffles=n_sh, n_strategies=len(strategies))
    gg.rt._init_worker(strategies, cfg, gp)
    rows = []
    for sh in range(n_sh):
        seed = gg.ur.coordinate_seed(gg.RandomPurpose.TOURNAMENT_SHUFFLE, root_seed=root, k=k, shuffle_index=sh, dtype=np.uint32)
        task = gg.rt.ShuffleTask(root_seed=root, k=k, shuffle_index=sh, shuffle_seed=int(seed), deterministic_batch_id=sh // 8)
        rows.extend(gg.rt._play_one_shuffle(task, collect_rows=True)[3])
    table = simulation_rows_to_table(rows, k)
    for seat in range(k + 1, (pad_to or k) + 1):  # the combined table's empty seats
        table = table.append_column(f"P{seat}_strategy", pa.nulls(table.num_rows, table.schema.field("P1_strategy").type))
        table = table.append_column(f"P{seat}_score", pa.nulls(table.num_rows, table.schema.field("P1_score").type))
    return rows, table


def encode(table: pa.Table) -> dict:
    """Schema (name, Arrow type) and column values; floats as float.hex, NaN as "nan", nulls as None."""
    cols = {}
    for name in table.schema.names:
        values = table.column(name).to_pylist()
        cols[name] = [v.hex() if isinstance(v, float) and v == v else ("nan" if isinstance(v, float) else v) for v in values]
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def k_frame(k, path, stage_dir, thresholds):
    captured = []
    orig = gs._write_scoped_game_stats, gs.write_stage_done, gs.resolved_code_identity_sha256
    gs._write_scoped_game_stats = lambda cfg, frame, *a, **kw: captured.append(frame.copy())
    gs.write_stage_done = lambda *a, **kw: None
    gs.resolved_code_identity_sha256 = lambda cfg: "golden"  # (only names the stage's resume checkpoint)
    try:
        gs._compute_k_game_stats(cfg=AppConfig(), k=k, input_path=path, stage_dir=stage_dir, thresholds=tuple(thresholds),
                                 config_sha=None, stage_config_sha="golden", cache_key_version=1)
    finally:
        gs._write_scoped_game_stats, gs.write_stage_done, gs.resolved_code_identity_sha256 = orig
    assert len(captured) == 1
    return pa.Table.from_pandas(captured[0], preserve_index=False)


def case(name, strategies, root, ks, n_sh, target, overrides=(), max_rounds=200, thresholds=(500, 1000), rare_target=10_000, pad_to=None):
    cells, per_n = [], []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for k in ks:
            ov = [o for o in overrides if o[1] == k]
            rows, table = simulate(strategies, k, root, n_sh, target, max_rounds, ov, pad_to)
            path = tmp / f"{k}p.parquet"
            pq.write_table(table, path)
            per_n.append((k, path))
            frame = k_frame(k, path, tmp / "stage", thresholds)
            cells.append({"k": k, "n_shuffles": n_sh, "overrides": [list(x) for x in ov],
                          "safety_limit_games": sum(1 for r in rows if r["termination_status"] != "completed"),
                          "game_stats": encode(frame)})
        out = tmp / "rare" / "rare_events.parquet"
        out.parent.mkdir()
        gs._rare_event_flags(per_n, cfg=None, thresholds=tuple(thresholds), target_score=rare_target, output_path=out, codec="snappy")
        rare = pq.read_table(out) if out.exists() else None
        strategy_arrow = str(gs._strategy_arrow_type(per_n))
    summary = None
    if rare is not None:
        level = rare.column("summary_level").to_pylist()
        keep = [i for i, v in enumerate(level) if v in ("strategy", "n_players")]
        summary = encode(rare.take(pa.array(keep, pa.int64())))
    return {"name": name, "root_seed": root, "target_score": target, "max_rounds": max_rounds, "thresholds": list(thresholds),
            "rare_target_score": rare_target, "pad_to": pad_to, "strategy_arrow": strategy_arrow,
            "strategies": [gg.strat_tuple(s) for s in strategies], "cells": cells, "rare_event_summary": summary}


def main():
    grid = gg.grid(score_thresholds=[300, 500, 700, 900], dice_thresholds=[1, 2], smart_five_opts=[False, True], smart_one_opts=[False, True],
                   include_stop_at=False, include_stop_at_heuristic=False, consider_score_opts=[True], consider_dice_opts=[True],
                   auto_hot_dice_opts=[True], run_up_score_opts=[False])
    s28, s12 = grid[:28], grid[:12]
    # (root, k, shuffle, game, max_rounds): games cut short by the safety limit
    safety = ((3, 2, 0, 1, 1), (3, 2, 1, 4, 2), (3, 2, 2, 0, 3), (3, 3, 0, 2, 1), (3, 3, 3, 1, 2), (3, 3, 4, 3, 4))
    out = {"cases": [
        case("k1247", s28, 7, (1, 2, 4, 7), 4, 10_000),
        case("safety_limit", s12, 3, (2, 3), 5, 3000, overrides=safety),
        case("pad12", s12, 9, (4,), 6, 4000, pad_to=12),
        case("thresholds", s12, 21, (2, 3), 6, 2000, thresholds=(50, 250, 777), rare_target=1500),
    ]}
    for c in out["cases"]:
        print(c["name"], [len(cell["game_stats"]["columns"]["summary_level"]) for cell in c["cells"]],
              [cell["safety_limit_games"] for cell in c["cells"]],
              None if c["rare_event_summary"] is None else len(c["rare_event_summary"]["columns"]["summary_level"]))
    gg._dump(out, open(gg.OUT / "game_stats_vectors.json", "w"))
    print((gg.OUT / "game_stats_vectors.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
