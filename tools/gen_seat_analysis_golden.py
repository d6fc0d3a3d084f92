"""TEST INFRASTRUCTURE ONLY — write tests/golden/seat_analysis_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The seat-analysis stage of the reference by its OWN code over rows it simulated (``gen_game_stats_golden.simulate`` with the
case's batch size): one parquet file per k in (batch, shuffle, game) order -> ``_iter_seat_count_tables`` -> ``_within_k_frames``
-> ``_standardized_frames`` (equal-k and a declared mapping) and ``_game_diagnostics``; for k = 2 ``_MirroredPartitionWriter`` per
(batch, partition) with 1 and with 3 partitions, whose shard rows are recorded and summed by pair the way
``_write_mirrored_diagnostic`` sums them.  Floats are recorded as ``float.hex``.

    python tools/gen_seat_analysis_golden.py [--time]
"""
from __future__ import annotations

import sys
import tempfile
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
sys.path.insert(0, str(HERE))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pandas as pd  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402
from farkle.analysis import seat_analysis as sa  # noqa: E402
from farkle.config import AppConfig, KAggregationConfig  # noqa: E402
from farkle.simulation.simulation import simulation_rows_to_table  # noqa: E402
from farkle.utils.partitioned_stage import PartitionedUnit  # noqa: E402

SHARD_SUMS = ("paired_mirrored_games", "p1_win_difference_sum", "games_completed", "games_safety_limit", "unpaired_forward_games",
              "unpaired_reverse_games")


def simulate(strategies, k, root, n_sh, spb, target, max_rounds, overrides):
    gp = gg.GameProfile(default_target_score=target, default_max_rounds=max_rounds,
                        tournament_max_rounds_overrides=tuple(gg.TournamentMaxRoundsOverride(*o) for o in overrides))
    cfg = gg.rt.TournamentConfig(n_players=k, num_shuffles=n_sh, n_strategies=len(strategies))
    gg.rt._init_worker(strategies, cfg, gp)
    rows = []
    for sh in range(n_sh):
        seed = gg.ur.coordinate_seed(gg.RandomPurpose.TOURNAMENT_SHUFFLE, root_seed=root, k=k, shuffle_index=sh, dtype=np.uint32)
        task = gg.rt.ShuffleTask(root_seed=root, k=k, shuffle_index=sh, shuffle_seed=int(seed), deterministic_batch_id=sh // spb)
        rows.extend(gg.rt._play_one_shuffle(task, collect_rows=True)[3])
    return rows, simulation_rows_to_table(rows, k)


def encode(table: pa.Table) -> dict:
    cols = {}
    for name in table.schema.names:
        values = table.column(name).to_pylist()
        cols[name] = [v.hex() if isinstance(v, float) and v == v else ("nan" if isinstance(v, float) else v) for v in values]
    return {"schema": [[f.name, str(f.type)] for f in table.schema], "columns": cols}


def frame(df: pd.DataFrame) -> dict:
    return encode(pa.Table.from_pandas(df, preserve_index=False))


def mirrored(path: Path, tmp: Path, root: int, batches: list[int], partitions: int) -> list[dict]:
    """The shard rows of every (batch, partition) unit, in unit order."""
    writer = sa._MirroredPartitionWriter(source=str(path), columns=tuple(sa._source_columns(2)), max_batch_bytes=1 << 20, max_records=1 << 20)
    out = []
    for batch in batches:
        for part in range(partitions):
            shard = tmp / f"mirror_{partitions}_{batch}_{part}.parquet"
            writer(PartitionedUnit((root, batch, part, partitions), shard.name), shard)
            out.extend(pq.read_table(shard).to_pylist())
    return out


def pair_rows(shard_rows: list[dict], root: int) -> list[dict]:
    """Shard rows summed by (root, a, b) in ascending key order; the mean as the final frame's one division."""
    totals: dict = defaultdict(lambda: [0] * 6)
    for r in shard_rows:
        cell = totals[(r["root_seed"], r["strategy_a"], r["strategy_b"])]
        for i, name in enumerate(SHARD_SUMS):
            cell[i] += r[name]
    rows = []
    for (rt, a, b), (matched, difference, completed, safety, forward, reverse) in sorted(totals.items()):
        mean = difference / matched if matched else None
        rows.append({"root_seed": rt, "k": 2, "strategy_a": a, "strategy_b": b, "paired_mirrored_games": matched,
                     "games_attempted": completed + safety, "games_completed": completed, "games_safety_limit": safety,
                     "unpaired_forward_games": forward, "unpaired_reverse_games": reverse,
                     "mean_p1_win_difference": None if mean is None else mean.hex()})
    return rows


def mirror_coverage(rows, spb) -> dict:
    """What the k = 2 data exercise of the pairing rule (main() asserts every entry over the cases)."""
    seg: dict = defaultdict(list)
    for r in rows:
        a, b = sorted((r["P1_strategy"], r["P2_strategy"]))
        if r["termination_status"] != "completed":
            seg[(r["shuffle_index"] // spb, a, b)].append((2, 0))
        else:
            seg[(r["shuffle_index"] // spb, a, b)].append((int(r["P1_strategy"] == b), int(r["winner_seat"] == "P1")))
    both_unequal = single = safety = order_matters = False
    for games in seg.values():
        f = [p for o, p in games if o == 0]
        rv = [p for o, p in games if o == 1]
        m = min(len(f), len(rv))
        both_unequal |= bool(f) and bool(rv) and len(f) != len(rv)
        single |= (bool(f) != bool(rv))
        safety |= any(o == 2 for o, _ in games)
        for seq in (f, rv):
            order_matters |= m >= 2 and len(seq) > m and sum(seq[:m]) != sum(seq[-m:])
    return {"both orientations with nF != nR": both_unequal, "a single orientation": single, "a safety-limit game": safety,
            "first m and last m games of an orientation differ": order_matters}


def case(name, strategies, root, ks, n_sh, spb, target, overrides=(), max_rounds=200, declared=None, timed=None):
    cells, by_k, population, sources = [], {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for k in ks:
            ov = [o for o in overrides if o[1] == k]
            rows, table = simulate(strategies, k, root, n_sh, spb, target, max_rounds, ov)
            path = tmp / f"{k}p.parquet"
            pq.write_table(table, path)
            sources[k] = path
            t0 = time.perf_counter()
            counts = pa.concat_tables(list(sa._iter_seat_count_tables(path, k)))
            t1 = time.perf_counter()
            if timed is not None:
                timed.append(("_iter_seat_count_tables", k, table.num_rows, t1 - t0))
            cells_seen = {(b, s, q) for b, s, q in zip(*(counts.column(c).to_pylist() for c in ("deterministic_batch_id", "strategy", "seat")))}
            n_batches = (n_sh + spb - 1) // spb
            absent = n_batches * len(strategies) * k - len(cells_seen)
            by_k[k], population[k] = sa._within_k_frames(counts.to_pandas(), k)
            cell = {"k": k, "n_shuffles": n_sh, "shuffles_per_batch": spb, "overrides": [list(x) for x in ov],
                    "safety_limit_games": sum(1 for r in rows if r["termination_status"] != "completed"), "absent_cells": absent,
                    "batch_counts": encode(counts), "by_k": frame(by_k[k]), "population_by_k": frame(population[k])}
            if k == 2:
                cell["coverage"] = mirror_coverage(rows, spb)
                batches = sorted({r["shuffle_index"] // spb for r in rows})
                t0 = time.perf_counter()
                one = mirrored(path, tmp, root, batches, 1)
                t1 = time.perf_counter()
                if timed is not None:
                    timed.append(("_MirroredPartitionWriter", k, table.num_rows, t1 - t0))
                three = mirrored(path, tmp, root, batches, 3)
                assert pair_rows(one, root) == pair_rows(three, root)
                cell["mirrored_shards"] = sorted(([r["deterministic_batch_id"], r["strategy_a"], r["strategy_b"]] + [r[n] for n in SHARD_SUMS]
                                                  for r in one))
                cell["mirrored_shards_3"] = sorted(([r["deterministic_batch_id"], r["strategy_a"], r["strategy_b"]] + [r[n] for n in SHARD_SUMS]
                                                    for r in three))
                cell["mirrored"] = pair_rows(one, root)
            cells.append(cell)
        ks_l = list(ks)
        cfg = AppConfig()
        std, mix = sa._standardized_frames(cfg, by_k, population, ks_l)
        out = {"standardized_equal_k": frame(std), "mixture_equal_k": frame(mix)}
        if declared:
            cfg = AppConfig()
            cfg.k_aggregation = KAggregationConfig(method="declared-mapping", k_weights=dict(declared))
            std, mix = sa._standardized_frames(cfg, by_k, population, ks_l)
            out.update(standardized_declared=frame(std), mixture_declared=frame(mix), declared_weights=[[k, float(w).hex()] for k, w in declared.items()])
        t0 = time.perf_counter()
        out["selfplay"] = frame(sa._game_diagnostics(sources))
        if timed is not None:
            timed.append(("_game_diagnostics", tuple(ks), sum(pq.read_metadata(p).num_rows for p in sources.values()), time.perf_counter() - t0))
    return {"name": name, "root_seed": root, "target_score": target, "max_rounds": max_rounds,
            "strategies": [gg.strat_tuple(s) for s in strategies], "cells": cells, **out}


def main():
    grid = gg.grid(score_thresholds=[300, 500, 700, 900], dice_thresholds=[1, 2], smart_five_opts=[False, True], smart_one_opts=[False, True],
                   include_stop_at=False, include_stop_at_heuristic=False, consider_score_opts=[True], consider_dice_opts=[True],
                   auto_hot_dice_opts=[True], run_up_score_opts=[False])
    s12, s4 = grid[:12], grid[:4]
    # (root, k, shuffle, game, max_rounds): games cut short by the safety limit (the list gen_game_stats_golden.py uses)
    safety = ((3, 2, 0, 1, 1), (3, 2, 1, 4, 2), (3, 2, 2, 0, 3), (3, 3, 0, 2, 1), (3, 3, 3, 1, 2), (3, 3, 4, 3, 4))
    timed = [] if "--time" in sys.argv else None
    out = {"cases": [
        case("s12_k1234", s12, 3, (1, 2, 3, 4), 20, 8, 3000, overrides=safety, declared={1: 0.1, 2: 0.4, 3: 0.3, 4: 0.2}, timed=timed),
        case("s4_k2", s4, 5, (2,), 48, 16, 3000, overrides=((5, 2, 3, 0, 1), (5, 2, 20, 1, 2), (5, 2, 40, 0, 1))),
    ]}
    k2 = [cell["coverage"] for c in out["cases"] for cell in c["cells"] if cell["k"] == 2]
    for what in k2[0]:
        assert any(cov[what] for cov in k2), f"no (batch, pair) segment with {what}"
    assert any(cell["absent_cells"] > 0 for c in out["cases"] for cell in c["cells"]), "every (batch, strategy, seat) cell is present"
    for c in out["cases"]:
        print(c["name"], [(cell["k"], cell["absent_cells"], cell["safety_limit_games"], len(cell.get("mirrored", ()))) for cell in c["cells"]])
    if timed:
        for what, k, n, sec in timed:
            print(f"reference {what} k={k}: {n} rows in {sec:.3f} s = {n / sec:,.0f} rows/s (one unrepeated run)")
    gg._dump(out, open(gg.OUT / "seat_analysis_vectors.json", "w"))
    print((gg.OUT / "seat_analysis_vectors.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
