"""TEST INFRASTRUCTURE ONLY — write tests/golden/rng_matchup_vectors.json by running the upstream Python reference in the build
container (oracle/ref_import.py; nothing here travels to the GPU machine except the JSON).

The matchup family of the reference's RNG diagnostics, by the reference's OWN code over rows it simulated: ``_play_one_shuffle``
rows -> ``simulation_rows_to_table`` padded to twelve ``P#_strategy`` columns as the combine stage pads them
(``expected_schema_for(12)``) -> ``_extract_batch_arrays`` -> ``_count_records`` / ``_observation_records`` ->
``_observation_sort_order`` -> ``_priority`` / ``_observation_histogram_bin`` -> the selection loop of
``_write_or_reuse_selection`` (analysis/rng_diagnostics.py:1606-1701, transcribed: the function itself reads partitioned
parquet files and writes sidecars) -> ``_OnlineMetric`` / ``_rows_for_online_group`` for the selected matchup groups.

    python tools/gen_rng_matchup_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))
import gen_golden as gg  # noqa: E402  (imports the reference through oracle/ref_import.py)

import pyarrow as pa  # noqa: E402
from farkle.analysis import rng_diagnostics as rd  # noqa: E402
from farkle.simulation.simulation import simulation_rows_to_table  # noqa: E402

MAX_PLAYERS = 12
LAGS = (1, 2, 5)


def simulate(strategies, k, root, n_sh, target, overrides):
    gp = gg.GameProfile(default_target_score=target, default_max_rounds=200,
                        tournament_max_rounds_overrides=tuple(gg.TournamentMaxRoundsOverride(*o) for o in overrides))
    cfg = gg.rt.TournamentConfig(n_players=k, num_shuffles=n_sh, n_strategies=len(strategies))
    gg.rt._init_worker(strategies, cfg, gp)
    rows = []
    for sh in range(n_sh):
        seed = gg.ur.coordinate_seed(gg.RandomPurpose.TOURNAMENT_SHUFFLE, root_seed=root, k=k, shuffle_index=sh, dtype=np.uint32)
        task = gg.rt.ShuffleTask(root_seed=root, k=k, shuffle_index=sh, shuffle_seed=int(seed), deterministic_batch_id=sh // 8)
        rows.extend(gg.rt._play_one_shuffle(task, collect_rows=True)[3])
    table = simulation_rows_to_table(rows, k)
    for seat in range(k + 1, MAX_PLAYERS + 1):  # the combined table's empty seats
        table = table.append_column(f"P{seat}_strategy", pa.nulls(table.num_rows, pa.int32()))
    return rows, table


def records_of(table, root):
    names = table.schema.names
    counts, obs, games = [], [], []
    for batch in table.to_batches(max_chunksize=37):  # several batches, as the stage streams them
        arrays = rd._extract_batch_arrays(batch, winner_col=rd._winner_column(set(names)), strat_cols=rd._seat_strategy_columns(None, names),
                                          expected_root_seed=root)
        counts.append(rd._count_records(arrays))
        obs.append(rd._observation_records(arrays))
        for i in range(batch.num_rows):
            games.append([int(arrays.k[i]), [int(v) for v in arrays.canonical_matchup[i] if v >= 0], str(int(arrays.matchup_id[i]))])
    return rd._reduce_count_array(np.concatenate(counts)), np.concatenate(obs), games


def selection(count_records, cap_cfg, minimum, lags, partitions):
    """The loop of _write_or_reuse_selection over the eligibility rows (count records + _priority + eligible)."""
    cap = rd._effective_max_matchup_groups(cap_cfg)
    mp = len([n for n in count_records.dtype.names if n.startswith("p")])
    top_dtype = rd._priority_key_dtype(mp)
    group_type = count_records["group_type"]
    observations = count_records["count"]
    eligible = observations >= minimum
    totals, eligible_totals, histogram = {}, {}, {}
    for value, label in ((rd._GROUP_STRATEGY, "strategy"), (rd._GROUP_MATCHUP, "matchup")):
        mask = group_type == value
        totals[label] = int(np.count_nonzero(mask))
        eligible_totals[label] = int(np.count_nonzero(mask & eligible))
        bins = rd._observation_histogram_bin(observations[mask], minimum)
        for b, c in zip(*np.unique(bins, return_counts=True)):
            histogram[(label, int(b))] = histogram.get((label, int(b)), 0) + int(c)
    mask = (group_type == rd._GROUP_MATCHUP) & eligible
    top = np.empty(int(np.count_nonzero(mask)), dtype=top_dtype)
    prio = rd._priority(count_records)
    for name in top_dtype.names:
        top[name] = (prio if name == "priority" else count_records[name])[mask]
    top = top[rd._priority_sort_order(top)]
    cutoff, capped = None, 0
    if cap is not None and eligible_totals["matchup"] > cap:
        top = top[:cap]
        cutoff = rd._priority_tuple(top[-1])
        capped = eligible_totals["matchup"] - cap
    below = totals["strategy"] + totals["matchup"] - eligible_totals["strategy"] - eligible_totals["matchup"]
    report = {
        "selection_schema_version": 1, "method_version": rd._DIAGNOSTIC_METHOD_VERSION, "partition_count": partitions,
        "minimum_usable_observations": minimum, "normalized_lags": list(lags), "effective_matchup_group_cap": cap,
        "total_candidate_groups": totals["strategy"] + totals["matchup"], "candidate_strategy_groups": totals["strategy"],
        "candidate_matchup_groups": totals["matchup"], "eligible_groups": eligible_totals["strategy"] + eligible_totals["matchup"],
        "eligible_strategy_groups": eligible_totals["strategy"], "eligible_matchup_groups": eligible_totals["matchup"],
        "selected_strategy_groups": eligible_totals["strategy"], "selected_matchup_groups": eligible_totals["matchup"] - capped,
        "below_minimum_observation_groups": below, "deterministically_capped_groups": capped,
        "exclusion_reasons": {"below_minimum_usable_observations": below, "deterministic_priority_cap": capped},
        "observation_count_distribution": [{"summary_level": label, "bin": rd._histogram_label(code, minimum), "groups": c}
                                           for (label, code), c in sorted(histogram.items())],
        "priority_cutoff": list(cutoff) if cutoff is not None else None,
        "completeness_status": "blocked_by_cap" if capped else "planned_complete",
    }
    report["selected_groups"] = int(report["selected_strategy_groups"]) + int(report["selected_matchup_groups"])
    keep = {tuple(int(r[n]) for n in top_dtype.names[1:]) for r in top}
    return report, keep


def stats_rows(observations, keep, lags):
    """_write_stats_partition over the selected matchup groups' observations, in _observation_sort_order."""
    rec = observations[observations["group_type"] == rd._GROUP_MATCHUP]
    rec = rec[rd._observation_sort_order(rec)]
    rows, current, rounds = [], None, None
    for record in rec:
        identity = rd._group_identity(record, rec.dtype)
        if identity != current:
            if current is not None and current in keep:
                rows.extend(rd._rows_for_online_group(current, lags=lags, rounds=rounds, wins=None))
            current, rounds = identity, rd._OnlineMetric(lags)
        rounds.push(float(record["n_rounds"]))
    if current is not None and current in keep:
        rows.extend(rd._rows_for_online_group(current, lags=lags, rounds=rounds, wins=None))
    return rows


def case(name, strategies, root, ks, n_sh, target, overrides, cap, partitions=4):
    counts, obs, games, cells = [], [], [], []
    for k in ks:
        ov = [o for o in overrides if o[1] == k]
        rows, table = simulate(strategies, k, root, n_sh, target, ov)
        c, o, g = records_of(table, root)
        counts.append(c)
        obs.append(o)
        cells.append({"k": k, "n_shuffles": n_sh, "games": g, "overrides": [list(x) for x in ov],
                      "safety_limit_games": sum(1 for r in rows if r["termination_status"] != "completed")})
    minimum = min(LAGS) + 2
    report, keep = selection(rd._reduce_count_array(np.concatenate(counts)), cap, minimum, LAGS, partitions)
    return {"name": name, "root_seed": root, "target_score": target, "max_rounds": 200, "max_players": MAX_PLAYERS,
            "rng_max_matchup_groups": cap, "rng_diagnostic_partitions": partitions, "strategies": [gg.strat_tuple(s) for s in strategies],
            "cells": cells, "report": report, "rows": stats_rows(np.concatenate(obs), keep, LAGS)}


def main():
    small = gg.grid(score_thresholds=[300, 500, 700], dice_thresholds=[1, 2], smart_five_opts=[False, True], smart_one_opts=[False], include_stop_at=False, include_stop_at_heuristic=False,
                    consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[False])
    wide = gg.grid(score_thresholds=[300, 500, 700], dice_thresholds=[1, 2], smart_five_opts=[False, True], smart_one_opts=[False, True], include_stop_at=False, include_stop_at_heuristic=False,
                   consider_score_opts=[True], consider_dice_opts=[True], auto_hot_dice_opts=[True], run_up_score_opts=[False])
    small, wide = small[:12], wide[:24]  # (the first strategies of each grid)
    overrides = ((11, 2, 3, 1, 2), (11, 3, 5, 0, 1))  # (root, k, shuffle, game, max_rounds): two safety-limit games
    out = {"lags": list(LAGS), "cases": [
        case("k234", small, 11, (2, 3, 4), 30, 1000, overrides, None),
        case("k234_capped", small, 11, (2, 3, 4), 30, 1000, overrides, 5),
        case("k12_singletons", wide, 5, (12,), 3, 1000, (), None),
    ]}
    for c in out["cases"]:
        print(c["name"], c["report"]["completeness_status"], c["report"]["eligible_matchup_groups"], len(c["rows"]))
    gg._dump(out, open(gg.OUT / "rng_matchup_vectors.json", "w"))
    print((gg.OUT / "rng_matchup_vectors.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
