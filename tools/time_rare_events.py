"""Cost of the rare-event passes on the device (``fk_tournament_run_rare_events``: second-score record + gather, and the ordered
compaction of the flagged games: count, scan, scatter) beyond ``fk_tournament_run_game_stats`` on the same ranges, at the shapes
of bench configs 2 and 3.

Per shape, after one warm-up of each call, ``--reps`` (default 7) rounds of: the game-stats call (the entry point as it was), the
histograms-only rare-events call, the rare-events call with the default fixed thresholds (500, 1000) / target 10 000, and the
quantile-mode pair (histograms-only pass, thresholds resolved from it at ``rare_event_margin_quantile = 0.01``, the replay that
collects the games).  From the engine's HIP events (``Engine.timing``) each call's time beyond its game kernel
(``total_ms - play_ms``) is kept; the tool reports min / median / max of those and of the differences to the game-stats call of the
same round, and the host wall time of the events calls (which includes copying the list).  Kernel-level times come from a run of
this tool under ``rocprofv3 --kernel-trace --stats``.

    python tools/time_rare_events.py [config2|config3|all] [--reps N] [--out profiles/rare_events_timing.jsonl]
"""
from __future__ import annotations

import json
import statistics
import sys
import time
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
    return out


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def main() -> None:
    from farkle_ii_amd import rare_events as rev
    from farkle_ii_amd.engine import get_engine

    which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "all"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    eng = get_engine()
    info = eng.device_info()
    lines = []
    for label, table, k, root, n_sh in shapes(which):
        n_games = n_sh * (len(table) // k)
        cap = n_games // 4  # room for every list below: no call is replayed for capacity

        def timed(fn):
            t0 = time.perf_counter()
            res = fn()
            wall = (time.perf_counter() - t0) * 1e3
            t = eng.timing()
            return res, t["total_ms"] - t["play_ms"], t["play_ms"], wall

        calls = {
            "game_stats": lambda: eng.tournament_game_stats(table, k, root, 0, n_sh),
            "histograms_only": lambda: eng.tournament_rare_events(table, k, root, 0, n_sh, want_events=False),
            "fixed": lambda: eng.tournament_rare_events(table, k, root, 0, n_sh, thresholds=(500, 1000), event_capacity=cap, retry=False),
        }
        first = calls["histograms_only"]()  # (warm-up, and the histograms the quantile is resolved from)
        thr, target = rev.resolve_rare_event_thresholds({k: rev.RareEventSummary.from_engine(first, k)}, (500, 1000), 10_000, 0.01, None)
        calls["quantile_replay"] = lambda: eng.tournament_rare_events(table, k, root, 0, n_sh, rare_target_score=target, thresholds=thr,
                                                                      event_capacity=cap, retry=False)
        for fn in calls.values():
            fn()
        post = {name: [] for name in calls}
        play = {name: [] for name in calls}
        wall = {name: [] for name in calls}
        events = {}
        for _ in range(reps):
            for name, fn in calls.items():
                res, p, g, w = timed(fn)
                post[name].append(p)
                play[name].append(g)
                wall[name].append(w)
                if "rare_events" in res:
                    events[name] = res["rare_events"]["events"]
        beyond = {name: [a - b for a, b in zip(post[name], post["game_stats"])] for name in calls if name != "game_stats"}
        line = {"shape": label, "k": k, "strategies": len(table), "shuffles": n_sh, "games": n_games, "device": info["arch"], "reps": reps,
                "quantile_thresholds": list(thr), "events": events,
                "post_ms": {name: spread(v) for name, v in post.items()}, "play_ms": {name: spread(v) for name, v in play.items()},
                "beyond_game_stats_ms": {name: spread(v) for name, v in beyond.items()},
                "wall_ms": {name: spread(v) for name, v in wall.items()},
                "quantile_mode_post_ms": spread([a + b for a, b in zip(post["histograms_only"], post["quantile_replay"])]),
                "quantile_mode_total_over_fixed": round(
                    statistics.median([a + b + c + d for a, b, c, d in zip(post["histograms_only"], play["histograms_only"],
                                                                           post["quantile_replay"], play["quantile_replay"])])
                    / statistics.median([a + b for a, b in zip(post["fixed"], play["fixed"])]), 3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
