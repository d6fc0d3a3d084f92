"""Cost of the RNG diagnostics' matchup family on the device (``fk_tournament_run_matchups`` + ``fk_matchup_reduce``).

Per shape: the lag-mode tournament call without and with the matchup records (the difference is the key post-pass and the
records' copy to the host), the game kernel's own time, the device reduce (sort, segments, selection, lag sums) and the host
selection + rows.  Shapes: bench config 2 (k = 2, 64 strategies, 10^7 games) and the production sweep (the default
5 160-strategy grid, 4 300 shuffles at k = 2, 3, 4, 5, 6, 8, 10, 12, root 102: configs/bench_mega_rows_off.yaml).  Kernel-level
times come from a run under ``rocprofv3 --kernel-trace --stats``.

    python tools/time_rng_matchups.py [config2|mega|all] [--reps N]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

LAGS = (1, 2, 5)


def shapes(which: str):
    from bench import grid64
    from tools.time_config import table_for

    out = []
    if which in ("config2", "all"):
        out.append(("config2", grid64(), 2, 42, 312_500))
    if which in ("mega", "all"):
        t = table_for(5160)
        out += [(f"mega_k{k}", t, k, 102, 4300) for k in (2, 3, 4, 5, 6, 8, 10, 12)]
    return out


def main() -> None:
    from farkle_ii_amd import rng_matchups as rm
    from farkle_ii_amd.engine import get_engine

    which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "all"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 2
    eng = get_engine()
    groups = []
    total = {"lags_s": 0.0, "matchups_s": 0.0, "play_ms": 0.0, "reduce_s": 0.0}
    for label, table, k, root, n_sh in shapes(which):
        ids = np.arange(len(table), dtype=np.int32)
        best = {}
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.tournament_lags(table, k, root, 0, n_sh, LAGS)
            t1 = time.perf_counter()
            play_lags = eng.timing()["play_ms"]
            res = eng.tournament_matchups(table, k, root, 0, n_sh, LAGS, ids, 12)
            t2 = time.perf_counter()
            play_m = eng.timing()["play_ms"]
            red = eng.matchup_reduce(res["matchups"], k, LAGS, rm.DEFAULT_MAX_MATCHUP_GROUPS)
            t3 = time.perf_counter()
            g = rm.MatchupGroups.from_reduce(red, ids, 12, rm.DEFAULT_MAX_MATCHUP_GROUPS)
            t4 = time.perf_counter()
            cur = {"lags_s": t1 - t0, "matchups_s": t2 - t1, "play_ms_lags": play_lags, "play_ms": play_m, "reduce_s": t3 - t2,
                   "host_groups_s": t4 - t3}
            best = cur if not best or cur["matchups_s"] + cur["reduce_s"] < best["matchups_s"] + best["reduce_s"] else best
        groups.append((label, g, rm.StrategyFamily(k, len(table), n_sh)))
        n_games = len(res["matchups"]["digest"])
        line = {"shape": label, "k": k, "strategies": len(table), "games": n_games, "candidate_groups": red["candidate_groups"],
                "eligible_groups": red["eligible_groups"], **{key: round(v, 4) for key, v in best.items()},
                "matchup_extra_s": round(best["matchups_s"] - best["lags_s"], 4)}
        for key in total:
            total[key] += best[key]
        print(json.dumps(line), flush=True)
    t0 = time.perf_counter()
    sweep = [x for x in groups if x[0].startswith("mega")] or groups  # one root's selection across its player counts
    rows, report = rm.select([x[1] for x in sweep], [x[2] for x in sweep], LAGS, rm.DEFAULT_MAX_MATCHUP_GROUPS, 1)
    t_sel = time.perf_counter() - t0
    print(json.dumps({"shape": f"{which}_total", **{key: round(v, 4) for key, v in total.items()}, "select_rows_s": round(t_sel, 4),
                      "matchup_rows": len(rows), "eligible_matchup_groups": report["eligible_matchup_groups"]}), flush=True)


if __name__ == "__main__":
    main()
