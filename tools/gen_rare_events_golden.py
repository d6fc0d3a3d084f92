"""TEST INFRASTRUCTURE ONLY — write tests/golden/rare_events_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The rare-event shards of the reference's game-stats stage by its OWN code over rows it simulated (as
tools/gen_game_stats_golden.py simulates them): per case, one parquet file per k written with SMALL ROW GROUPS, then

* ``_resolve_rare_event_thresholds`` with the case's margin quantile / target rate -> the resolved thresholds and target;
* ``_build_rare_event_summary_shard`` per k under the resolved values with a small ``max_batch_bytes``: the shard's game rows
  and counters, and the batch lengths its reader produced (``iter_parquet_tables_by_bytes`` wrapped to record them), so the
  multi-batch seat-major order is pinned;
* ``_rare_event_details`` -> the details rows (its scanner's batch lengths over the same file are recorded too);
* ``_rare_event_flags`` -> the final ``rare_events.parquet`` (game rows of every k + summary rows).

Per case set it asserts that at least one game falls in each class: multi-target only, margin only, both, flagged
safety-limit, unflagged.  Floats are recorded as ``float.hex``; only data the reference wrote is recorded.

    python tools/gen_rare_events_golden.py
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import gen_game_stats_golden as base  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pyarrow.dataset as ds  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402

gg, gs = base.gg, base.gs
ROW_GROUP = 5           # games per row group of the per-k files
MAX_BATCH_BYTES = 600   # the shard reader's byte budget: a few row groups per batch


def recorded_batches(fn):
    """Run ``fn`` with the reference's batch reader wrapped: the lengths of the tables it yielded, by file name."""
    seen: dict[str, list[int]] = {}
    orig = gs.iter_parquet_tables_by_bytes

    def wrapped(path, *a, **kw):
        for item in orig(path, *a, **kw):
            seen.setdefault(Path(path).name, []).append(int(item[2].num_rows))
            yield item

    gs.iter_parquet_tables_by_bytes = wrapped
    try:
        fn()
    finally:
        gs.iter_parquet_tables_by_bytes = orig
    return seen


def encode(table) -> dict:
    """``gen_game_stats_golden.encode`` with every column that has long runs (constant strings, flags, per-game values repeated
    over the seats' rows) stored as ``{"runs": [[value, count], ...]}``."""
    enc = base.encode(table)
    for name, values in enc["columns"].items():
        runs = []
        for v in values:
            if runs and runs[-1][0] == v and type(runs[-1][0]) is type(v):
                runs[-1][1] += 1
            else:
                runs.append([v, 1])
        if len(json.dumps(runs)) < len(json.dumps(values)):
            enc["columns"][name] = {"runs": runs}
    return enc


def classes(rows, thresholds, target) -> dict:
    """How many games of ``rows`` (the reference's row dicts) fall in each class under the resolved values."""
    out = {"multi_only": 0, "margin_only": 0, "both": 0, "flagged_safety_limit": 0, "unflagged": 0}
    for r in rows:
        scores = sorted(v for name, v in r.items() if name.startswith("P") and name.endswith("_score") and v is not None)
        completed = r["termination_status"] == "completed"
        multi = sum(1 for v in scores if v >= target) >= 2
        margin = completed and len(scores) >= 2 and any(scores[-1] - scores[-2] <= t for t in thresholds)
        if not completed and (multi or margin):
            out["flagged_safety_limit"] += 1
        if multi and margin:
            out["both"] += 1
        elif multi:
            out["multi_only"] += 1
        elif margin:
            out["margin_only"] += 1
        else:
            out["unflagged"] += 1
    return out


def case(name, strategies, root, ks, n_sh, target, overrides=(), max_rounds=200, thresholds=(500, 1000), rare_target=10_000, pad_to=None,
         margin_quantile=None, target_rate=None):
    cells, per_n, all_rows = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for k in ks:
            ov = [o for o in overrides if o[1] == k]
            rows, table = base.simulate(strategies, k, root, n_sh, target, max_rounds, ov, pad_to)
            path = tmp / f"{k}p.parquet"
            pq.write_table(table, path, row_group_size=ROW_GROUP)
            per_n.append((k, path))
            all_rows.extend(rows)
            # (the details pass reads through a dataset scanner: its batches never cross a row group)
            scanned = [int(b.num_rows) for b in ds.dataset(path).scanner(batch_size=65_536).to_batches()]
            cells.append({"k": k, "n_shuffles": n_sh, "n_games": len(rows), "overrides": [list(x) for x in ov], "details_batches": scanned})
        res_thr, res_target = gs._resolve_rare_event_thresholds(per_n, thresholds=tuple(thresholds), target_score=rare_target,
                                                                margin_quantile=margin_quantile, target_rate=target_rate)
        strategy_arrow = gs._strategy_arrow_type(per_n)
        for cell, (k, path) in zip(cells, per_n):
            shard, stats, done = tmp / f"shard_{k}.parquet", tmp / f"shard_{k}.json", tmp / f"shard_{k}.done"
            seen = recorded_batches(lambda: gs._build_rare_event_summary_shard(
                n_players=k, input_path=path, thresholds=res_thr, target_score=res_target, strategy_arrow=strategy_arrow, shard_path=shard,
                stats_path=stats, done_path=done, codec="snappy", config_sha="golden", run_config_sha=None, cache_key_version=1,
                publish_completion=False, max_batch_bytes=MAX_BATCH_BYTES))
            payload = json.loads(stats.read_text())
            fields = sorted(payload["global_sums"])  # (the counters of every strategy, one row each)
            cell.update(shard_batches=seen.get(path.name, []), shard=encode(pq.read_table(shard)),
                        shard_global_sums=payload["global_sums"],
                        shard_strategy_sums={"fields": fields, "strategy": [int(v) for v in sorted(payload["strategy_sums"], key=int)],
                                             "values": [[payload["strategy_sums"][sid][f] for f in fields]
                                                        for sid in sorted(payload["strategy_sums"], key=int)]})
        details = tmp / "details" / "rare_events_details.parquet"
        details.parent.mkdir()
        gs._rare_event_details(per_n, thresholds=res_thr, target_score=res_target, output_path=details, codec="snappy")
        out = tmp / "rare" / "rare_events.parquet"
        out.parent.mkdir()
        flags_seen = recorded_batches(lambda: gs._rare_event_flags(per_n, cfg=None, thresholds=res_thr, target_score=res_target,
                                                                   output_path=out, codec="snappy"))
        for cell, (k, path) in zip(cells, per_n):
            cell["flags_batches"] = flags_seen.get(path.name, [])
        result = {"name": name, "root_seed": root, "target_score": target, "max_rounds": max_rounds, "thresholds": list(thresholds),
                  "rare_target_score": rare_target, "margin_quantile": margin_quantile, "target_rate": target_rate,
                  "resolved_thresholds": [int(t) for t in res_thr], "resolved_target_score": int(res_target), "pad_to": pad_to,
                  "strategy_arrow": str(strategy_arrow), "strategies": [gg.strat_tuple(s) for s in strategies], "cells": cells,
                  "classes": classes(all_rows, res_thr, res_target),
                  "details": encode(pq.read_table(details)) if details.exists() else None,
                  "rare_events": encode(pq.read_table(out)) if out.exists() else None}
    return result


def main():
    grid = gg.grid(score_thresholds=[300, 500, 700, 900], dice_thresholds=[1, 2], smart_five_opts=[False, True], smart_one_opts=[False, True],
                   include_stop_at=False, include_stop_at_heuristic=False, consider_score_opts=[True], consider_dice_opts=[True],
                   auto_hot_dice_opts=[True], run_up_score_opts=[False])
    s28, s12 = grid[:28], grid[:12]
    # (root, k, shuffle, game, max_rounds): games cut short by the safety limit
    safety = tuple((3, k, sh, g, r) for k, games in ((2, 6), (3, 4)) for sh in range(4) for g, r in ((0, 3), (games - 1, 4)))
    out = {"cases": [
        case("k1247", s28, 7, (1, 2, 4, 7), 3, 2000, rare_target=1800),
        case("safety_limit", s12, 3, (2, 3), 4, 3000, overrides=safety, rare_target=600),
        case("pad12", s12, 9, (4,), 4, 2000, pad_to=12, rare_target=1700),
        case("thresholds", s12, 21, (2, 3), 4, 2000, thresholds=(50, 250, 777), rare_target=1500),
        case("quantile_both", s12, 21, (2, 3), 4, 2000, rare_target=1500, margin_quantile=0.2, target_rate=0.25),
        case("quantile_margin", s12, 5, (2, 3), 3, 2000, rare_target=1900, margin_quantile=0.1),
        case("quantile_target", s12, 5, (2, 3), 3, 2000, thresholds=(100,), rare_target=1900, target_rate=0.1),
    ]}
    total = {}
    for c in out["cases"]:
        print(c["name"], c["resolved_thresholds"], c["resolved_target_score"], c["classes"],
              [(cell["k"], cell["shard_batches"], len(cell["shard"]["columns"]["summary_level"])) for cell in c["cells"]])
        for name, n in c["classes"].items():
            total[name] = total.get(name, 0) + n
    for name in ("multi_only", "margin_only", "both", "flagged_safety_limit", "unflagged"):
        assert total.get(name, 0) >= 1, f"no game of class {name}: change the seeds"
    assert any(len(cell["shard_batches"]) >= 2 for c in out["cases"] for cell in c["cells"]), "no multi-batch shard"
    gg._dump(out, open(gg.OUT / "rare_events_vectors.json", "w"))
    print((gg.OUT / "rare_events_vectors.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
