"""The graphs the dominance tests run on: designed decision classes, bounds and rates of every pair of a small table.

A case is a dictionary: ``n``, ``ids`` (strategy ids, ascending but NOT in string order — 8, 9, 10, .., 100, .. — so the tie-break
order ``rank`` matters), ``cls`` / ``low`` / ``high`` / ``rate`` / ``d_ab`` per pair in pair-id order, ``strategies`` (the inference's
per-strategy table, int64 ``[n, 12]``: games attempted / completed and the two viability flags are what the frames read),
``scores`` (``{id: tournament screening score}``) and ``delta``.  Distances are multiples of 2^-10, so equal ones are equal exactly.
``CASES`` maps a name to a builder; ``all_cases()`` builds each once."""
from __future__ import annotations

import functools

import numpy as np

DELTA = 0.03
PRACTICAL, STATISTICAL = "practical", "statistical"


def _pair_index(n: int) -> dict:
    from farkle_ii_amd import round_robin as rr

    _, i, j = rr.pair_ids(n)
    return {(int(a), int(b)): p for p, (a, b) in enumerate(zip(i, j))}


def build(n: int, edges, *, nonviable_pairs=(), not_eligible=(), seed: int = 1, distance=None) -> dict:
    """``edges``: ``(winner, loser, PRACTICAL | STATISTICAL)`` — at most one per unordered pair; every other pair is unresolved, the
    pairs of ``nonviable_pairs`` (unordered row pairs) have no test: class 6, NaN bounds and rate.  ``distance(winner, loser)`` gives a
    practical edge's distance beyond the threshold in units of 2^-10 (default: seeded, 1 .. 64)."""
    rng = np.random.default_rng(seed)
    index = _pair_index(n)
    n_pairs = n * (n - 1) // 2
    cls = np.full(n_pairs, 5, dtype=np.uint8)
    low, high = np.full(n_pairs, -0.01), np.full(n_pairs, 0.0125)
    jitter = rng.integers(-8, 9, size=n_pairs) / 1024.0
    low, high = low + jitter, high + jitter
    for winner, loser, kind in edges:
        a, b = min(winner, loser), max(winner, loser)
        p = index[(a, b)]
        if cls[p] != 5:
            raise ValueError(f"two edges for the pair ({a}, {b})")
        a_wins = winner == a
        if kind == PRACTICAL:
            units = int(rng.integers(1, 65)) if distance is None else int(distance(winner, loser))
            inner = DELTA + units / 1024.0  # the bound on the winner's side
            cls[p] = 0 if a_wins else 1
            low[p], high[p] = (inner, inner + 0.03125) if a_wins else (-inner - 0.03125, -inner)
        else:
            cls[p] = 2 if a_wins else 3
            low[p], high[p] = (0.0078125, 0.046875) if a_wins else (-0.046875, -0.0078125)
    d_ab = 0.5 * (low + high)
    rate = 0.5 + d_ab
    for a, b in nonviable_pairs:
        p = index[(min(a, b), max(a, b))]
        if cls[p] != 5:
            raise ValueError(f"the pair ({a}, {b}) has an edge and no test")
        cls[p] = 6
        low[p] = high[p] = d_ab[p] = rate[p] = np.nan
    strategies = np.zeros((n, 12), dtype=np.int64)
    strategies[:, 7] = 4000 + rng.integers(0, 50, size=n)  # attempted
    strategies[:, 8] = strategies[:, 7] - rng.integers(0, 30, size=n)  # completed
    strategies[:, 10] = 1
    strategies[:, 11] = 1
    touched = sorted({int(v) for pair in nonviable_pairs for v in pair})
    strategies[touched, 11] = 0
    strategies[list(not_eligible), 10] = 0
    ids = 8 + np.arange(n, dtype=np.int64)
    scores = {int(s): float(v) for s, v in zip(ids, rng.integers(0, 8, size=n) / 8.0)}  # few values: ties reach the last sort key
    return {"n": n, "ids": ids, "cls": cls, "low": low, "high": high, "rate": rate, "d_ab": d_ab, "strategies": strategies, "scores": scores,
            "delta": DELTA}


def _kind(rng) -> str:
    return PRACTICAL if rng.random() < 0.5 else STATISTICAL


def sparse_random(n: int, seed: int) -> dict:
    """Mostly transitive — the smaller row wins six pairs in ten — with about one short back edge per node: many small components."""
    rng = np.random.default_rng(seed)
    back = {}
    for _ in range(n):
        i = int(rng.integers(0, n - 1))
        j = min(n - 1, i + 1 + int(rng.integers(0, 3)))
        back[(i, j)] = (j, i, _kind(rng))
    edges = list(back.values())
    for i in range(n):
        for j in range(i + 1, n):
            if (i, j) not in back and rng.random() < 0.6:
                edges.append((i, j, _kind(rng)))
    return build(n, edges, seed=seed)


def dense_random(n: int, seed: int) -> dict:
    """Nine pairs in ten directed, either way: one giant component."""
    rng = np.random.default_rng(seed)
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() < 0.9:
                edges.append((i, j, _kind(rng)) if rng.random() < 0.5 else (j, i, _kind(rng)))
    return build(n, edges, seed=seed)


def ring(nodes, kind=PRACTICAL) -> list:
    nodes = list(nodes)
    return [(a, b, kind) for a, b in zip(nodes, nodes[1:] + nodes[:1])]


def _winner_over_everyone(eligible: bool) -> dict:
    rng = np.random.default_rng(77)
    n = 20
    edges = [(3, v, PRACTICAL) for v in range(n) if v != 3]
    edges += [(i, j, _kind(rng)) if rng.random() < 0.5 else (j, i, _kind(rng)) for i in range(n) for j in range(i + 1, n) if 3 not in (i, j) and rng.random() < 0.7]
    return build(n, edges, seed=77, not_eligible=() if eligible else (3,))


CASES = {
    "n2_no_edge": lambda: build(2, []),
    "n2_one_edge": lambda: build(2, [(1, 0, PRACTICAL)]),
    "cycle3_and_tail": lambda: build(4, ring([0, 1, 2]) + [(2, 3, PRACTICAL)]),
    **{f"sparse_{n}": functools.partial(sparse_random, n, 100 + n) for n in (63, 64, 65, 128, 129)},
    **{f"dense_{n}": functools.partial(dense_random, n, 200 + n) for n in (63, 64, 65, 128, 129)},
    "component_across_a_word_boundary": lambda: build(70, ring([62, 63, 64, 65]) + [(10, 62, STATISTICAL), (65, 69, PRACTICAL)]),
    "total_order_100": lambda: build(100, [(i, j, PRACTICAL if (i + j) % 3 else STATISTICAL) for i in range(100) for j in range(i + 1, 100)]),
    "path_300": lambda: build(300, [(i, i + 1, PRACTICAL if i % 3 else STATISTICAL) for i in range(299)]),
    "ring_130": lambda: build(130, ring(range(130))),
    "two_rings_of_equal_length": lambda: build(12, ring(range(6)) + ring(range(6, 12))),
    "two_3_cycles_joined": lambda: build(6, ring([0, 1, 2]) + ring([3, 4, 5]) + [(2, 3, PRACTICAL)]),
    "statistical_component_without_practical_edge": lambda: build(6, ring([0, 1, 2], STATISTICAL) + [(3, 4, PRACTICAL), (2, 5, STATISTICAL)]),
    # ids 8 9 10 11 12 sort as strings 10 11 12 8 9: equal distances everywhere, both tie passes decide
    "equal_distances": lambda: build(5, ring(range(5)) + [(0, 2, PRACTICAL), (3, 1, PRACTICAL), (4, 2, PRACTICAL)], distance=lambda w, l: 16),
    "equal_distance_pairs_of_extremes": lambda: build(7, ring(range(7)) + [(0, 3, PRACTICAL), (5, 2, STATISTICAL)], distance=lambda w, l: 8 if (w + l) % 2 else 40),
    "several_shortest_cycles": lambda: build(6, ring([0, 1, 2]) + ring([3, 4, 5]) + [(2, 3, PRACTICAL), (5, 0, PRACTICAL)]),
    "pairs_without_a_rate": lambda: build(9, ring([0, 1, 2, 3]) + [(4, 5, PRACTICAL), (6, 7, STATISTICAL)], nonviable_pairs=[(0, 8), (4, 8), (2, 7)]),
    "strategy_without_any_rate": lambda: build(6, ring([0, 1, 2]) + [(3, 4, PRACTICAL)], nonviable_pairs=[(5, v) for v in range(5)]),
    "winner_over_everyone": lambda: _winner_over_everyone(True),
    "winner_over_everyone_not_eligible": lambda: _winner_over_everyone(False),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    return CASES[name]()


def all_cases() -> dict:
    return {name: case(name) for name in CASES}


def class_counts(c: dict) -> np.ndarray:
    return np.bincount(c["cls"], minlength=7).astype(np.int64)


def inference_rows(c: dict) -> np.ndarray:
    """The pair rows ``Engine.rr_inference`` would hand ``dominance.edges_frame``: the fields that frame reads."""
    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd.backend import RR_PAIR_ROW_DTYPE

    pid, i, j = rr.pair_ids(c["n"])
    rows = np.zeros(len(pid), dtype=RR_PAIR_ROW_DTYPE)
    rows["pair_id"], rows["strategy_a"], rows["strategy_b"] = pid, i, j
    rows["decision_class"], rows["d_ab"], rows["simultaneous_d_low"], rows["simultaneous_d_high"] = c["cls"], c["d_ab"], c["low"], c["high"]
    rows["balanced_a_win_rate"] = c["rate"]
    return rows


# ---- a frame as comparable data: floats by bit pattern ----
def frame_records(frame) -> dict:
    """``{"columns", "dtypes", "rows"}`` of a pandas frame, every float as the hex of its bits (NaN included), None for a null object."""
    def cell(v):
        if v is None:
            return None
        if isinstance(v, (float, np.floating)):
            return "f:" + np.float64(v).tobytes().hex()
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        return str(v)

    return {"columns": [str(c) for c in frame.columns], "dtypes": [str(t) for t in frame.dtypes],
            "rows": [[cell(v) for v in row] for row in frame.itertuples(index=False, name=None)]}


def frame_digest(frame) -> dict:
    """A frame too large to keep value by value: its columns, dtypes, row count and the SHA-256 of ``frame_records``' rows."""
    import hashlib
    import json

    rec = frame_records(frame)
    text = json.dumps(rec["rows"], separators=(",", ":"), sort_keys=True)
    return {"columns": rec["columns"], "dtypes": rec["dtypes"], "n_rows": len(rec["rows"]), "sha256": hashlib.sha256(text.encode("utf-8")).hexdigest()}


FULL_ROWS_LIMIT = 40  # frames of at most this many rows are kept value by value in the golden file, larger ones as digests


def frame_golden(frame) -> dict:
    return frame_records(frame) if len(frame) <= FULL_ROWS_LIMIT else frame_digest(frame)
