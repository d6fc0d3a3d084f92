"""Cost of the game-stats stage on the device (``fk_tournament_run_game_stats``: the game-record pass and the per-strategy LDS
histogram gather), against the game kernel's time, at the shapes of bench configs 2, 3 and 6.

Per shape and repetition, from the engine's HIP events (``Engine.timing``): the counts-only tournament call, the stats-mode call
that writes the state store (``want_seat_stats``: what the all-player batches run), and the game-stats call.  The post-passes'
cost is the game-stats call's non-game-kernel time minus the counts-only call's (``post_ms``); the best repetition is kept.
Kernel-level times come from a run of this tool under ``rocprofv3 --kernel-trace --stats``.

    python tools/time_game_stats.py [config2|config3|config6|all] [--reps N] [--out profiles/game_stats_timing.jsonl]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def shapes(which: str):
    from bench import grid64
    from tools.time_config import table_for

    out = []
    if which in ("config2", "all"):
        out.append(("config2", grid64(), 2, 42, 312_500))
    if which in ("config3", "all"):
        out.append(("config3", table_for(5160), 4, 0, 77_520))
    if which in ("config6", "all"):  # 10^8 games split equally over the production player counts
        t = table_for(5160)
        out += [(f"config6_k{k}", t, k, 0, 12_500_000 // (5160 // k)) for k in (2, 3, 4, 5, 6, 8, 10, 12)]
    return out


def main() -> None:
    from farkle_ii_amd.engine import get_engine

    which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "all"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    info = eng.device_info()
    lines = []
    for label, table, k, root, n_sh in shapes(which):
        best = None
        for _ in range(reps):
            eng.tournament(table, k, root, 0, n_sh)
            a = eng.timing()
            eng.tournament(table, k, root, 0, n_sh, want_seat_stats=True, want_seat_ratios=False)
            b = eng.timing()
            res = eng.tournament_game_stats(table, k, root, 0, n_sh)
            c = eng.timing()
            cur = {"play_ms": a["play_ms"], "total_ms": a["total_ms"], "state_play_ms": b["play_ms"], "state_total_ms": b["total_ms"],
                   "game_stats_play_ms": c["play_ms"], "game_stats_total_ms": c["total_ms"],
                   "post_ms": (c["total_ms"] - c["play_ms"]) - (a["total_ms"] - a["play_ms"])}
            best = cur if best is None or cur["game_stats_total_ms"] < best["game_stats_total_ms"] else best
        line = {"shape": label, "k": k, "strategies": len(table), "shuffles": n_sh, "games": n_sh * (len(table) // k),
                "device": info["arch"], **{key: round(v, 3) for key, v in best.items()},
                "post_share_of_game_kernel": round(best["post_ms"] / best["game_stats_play_ms"], 4), "spilled": res["spilled"]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
