"""Cost of the dominance graph stage (``fk_dominance_graph``) on the device, on seeded synthetic decision classes.

Two table sizes — 150 strategies (the reference's finalists, 11 175 pairs) and 5 160 (the whole default grid, 13 310 220 pairs) — and
two draws each:

``transitive``  the smaller row wins six pairs in ten, half of them by practical dominance, and one node in fifty loses to a node up
                to three rows below it: a long condensation (many fronts), few and small cycle groups;
``tangled``     nine pairs in ten are directed, either way: one component holds nearly every node.

Per shape a warm-up and ``--reps`` (default 5) calls with ``adjacency`` null: the entry's HIP events (``fk_timing``: ``perm_ms`` the
edge kernel, ``seed_ms`` the closure, ``play_ms`` the whole device work) and the host clock around the call, min / median / max, and
what the graphs look like (components, fronts, cycle lengths).  No threshold is set.

``--reference`` (build container only: it imports the upstream reference through oracle/ref_import.py) times the reference's own
dominance statements on the two 150-strategy draws on the CPU and writes ``profiles/dominance_reference_cpu.json``; a later device run
copies those figures beside its own, for context only.

    python tools/time_dominance.py [--only 150|5160] [--reps N] [--commit ID] [--out profiles/dominance_timing.jsonl]
    python tools/time_dominance.py --reference
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "oracle")]
REFERENCE_FILE = ROOT / "profiles" / "dominance_reference_cpu.json"
DELTA = 0.03


def spread(values) -> dict:
    return {"min": round(min(values), 3), "median": round(statistics.median(values), 3), "max": round(max(values), 3)}


def draw(n: int, kind: str, seed: int = 11) -> dict:
    """Classes, simultaneous bounds and rates of every pair of an ``n``-row table."""
    from farkle_ii_amd import round_robin as rr

    rng = np.random.default_rng(seed + n)
    _, i, j = rr.pair_ids(n)
    pairs = len(i)
    practical = rng.random(pairs) < 0.5
    if kind == "transitive":
        directed = rng.random(pairs) < 0.6
        a_wins = np.ones(pairs, dtype=bool)
        back = (j - i <= 3) & (rng.random(pairs) < 1.0 / 50.0)
        directed |= back
        a_wins[back] = False
    else:
        directed = rng.random(pairs) < 0.9
        a_wins = rng.random(pairs) < 0.5
    cls = np.where(directed, np.where(practical, 0, 2) + np.where(a_wins, 0, 1), 5).astype(np.uint8)
    inner = DELTA + rng.integers(1, 4097, size=pairs) / 65536.0
    low = np.where(cls == 0, inner, np.where(cls == 1, -inner - 0.03, np.where(cls == 2, 0.008, np.where(cls == 3, -0.046, -0.01))))
    high = np.where(cls == 0, inner + 0.03, np.where(cls == 1, -inner, np.where(cls == 2, 0.046, np.where(cls == 3, -0.008, 0.0125))))
    return {"n": n, "cls": cls, "low": low, "high": high, "rate": 0.5 + 0.5 * (low + high), "d_ab": 0.5 * (low + high), "delta": DELTA}


def shape_of(nodes: np.ndarray) -> dict:
    out = {}
    for g, name in enumerate(("practical", "statistical")):
        heads = nodes["component"][:, g] == np.arange(len(nodes))
        if not np.array_equal(nodes["front"][:, g], nodes["front"][nodes["component"][:, g], g]):
            raise SystemExit(f"{name}: a component's nodes lie on different fronts")
        out[name] = {"edges": int(nodes["wins"][:, g].sum()), "components": int(heads.sum()),
                     "cycle_groups": int((heads & (nodes["component_size"][:, g] > 1)).sum()),
                     "largest_component": int(nodes["component_size"][:, g].max()), "fronts": int(nodes["front"][:, g].max()),
                     "longest_shortest_cycle": int(nodes["cycle_length"][:, g].max())}
    return out


def device_runs(args) -> None:
    from farkle_ii_amd import dominance as dom
    from farkle_ii_amd.backend import Engine

    reference = json.loads(REFERENCE_FILE.read_text()) if REFERENCE_FILE.exists() else {}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with Engine(0) as eng:
        device = eng.device_info()["arch"]
        for n in (150, 5160):
            if args.only not in (None, n):
                continue
            rank = dom.rank_of_ids(8 + np.arange(n))
            for kind in ("transitive", "tangled"):
                d = draw(n, kind)
                stages = {"edges_ms": [], "closure_ms": [], "device_ms": [], "wall_ms": []}
                for rep in range(args.reps + 1):  # the first call warms up
                    t0 = time.perf_counter()
                    result = eng.dominance_graph(n, d["cls"], d["low"], d["high"], d["rate"], DELTA, rank=rank, want_adjacency=False)
                    wall = (time.perf_counter() - t0) * 1e3
                    t = eng.timing()
                    if rep:
                        for key, value in (("edges_ms", t["perm_ms"]), ("closure_ms", t["seed_ms"]), ("device_ms", t["play_ms"]), ("wall_ms", wall)):
                            stages[key].append(value)
                line = {"what": f"dominance_graph_{n}_{kind}", "strategies": n, "pairs": n * (n - 1) // 2, "reps": args.reps,
                        **{k: spread(v) for k, v in stages.items()}, "graphs": shape_of(result["nodes"]), "device": device, "commit": args.commit}
                if n <= 300:  # small enough for the host statement: the timed result is the right one
                    host = dom.graph(n, d["cls"], d["low"], d["high"], d["rate"], DELTA, rank=rank)
                    line["equals_host_statement"] = bool(result["nodes"].tobytes() == host["nodes"].tobytes()
                                                         and result["extremes"].tobytes() == host["extremes"].tobytes())
                key = f"{n}_{kind}"
                if key in reference:
                    line["reference_cpu_ms_for_context"] = reference[key]
                print(json.dumps(line), flush=True)
                with args.out.open("a") as fh:
                    fh.write(json.dumps(line) + "\n")


def reference_runs() -> None:
    import ref_import

    from tools import gen_dominance_golden as gen

    ref_import.import_reference()
    sys.setrecursionlimit(5000)
    out = {}
    for kind in ("transitive", "tangled"):
        d = draw(150, kind)
        n = d["n"]
        d["ids"] = 8 + np.arange(n, dtype=np.int64)
        d["strategies"] = np.tile(np.array([0] * 7 + [4000, 3990, 10, 1, 1], dtype=np.int64), (n, 1))
        d["scores"] = {int(s): 0.0 for s in d["ids"]}
        gen.reference_digest(d)  # imports and caches
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            gen.reference_digest(d)
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"150_{kind}"] = round(min(times), 1)
        print(f"reference, 150 strategies, {kind}: {out[f'150_{kind}']} ms", file=sys.stderr)
    REFERENCE_FILE.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, choices=(150, 5160))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "dominance_timing.jsonl")
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    if args.reference:
        reference_runs()
    else:
        device_runs(args)


if __name__ == "__main__":
    main()
