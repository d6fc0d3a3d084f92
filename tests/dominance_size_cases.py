"""Designed dominance graphs at the table sizes where the device kernels change shape (tests/test_dominance_size_host.py, _gpu.py): more
nodes than the front kernel has threads (1 025), more row words than a wave has lanes (4 097), every compile-time limit full (8 192).

The conventions are ``dominance_cases.build``'s — classes 0-3 for edges, 5 unresolved, 6 with NaN bounds and rate; bounds on the 2^-10
grid around ``DELTA``; ``rate = 0.5 + d_ab`` — but vectorised: the pair id is the closed form ``i (2n - i - 1) / 2 + j - i - 1``, no
dictionary of pairs is built.  A case is ``{"n", "ids", "cls", "low", "high", "rate", "delta", "edges"}``; ``edges`` is the list the case
was built from, ``(winner, loser, practical)`` as three arrays, and is what tests/dominance_sparse_oracle.py starts from.

``SIZE_CASES`` is separate from ``dominance_cases.CASES``, which stays tied to the reference-recorded golden file.

Strategy ids.  ``8 + arange(n)`` where nothing hangs on them.  ``thresholds`` and ``dense_band_4160`` use ``stepped_ids``: the same ids plus
a power of ten from the centre of every ring on, so that inside a ring the rows at and above the centre have one digit more than the
rows below it and sort, as strings, BEFORE them.  With plain ``8 + arange(n)`` the nine ids of a ring (68..76, 1028..1036, 4100..4108)
have equal length, the string order inside a ring is the table order, and no tie between two edges of a ring could tell ``rank`` from
the table order."""
from __future__ import annotations

import functools

import numpy as np

from dominance_cases import DELTA

RING = 9                       # nodes of a designed ring
THRESHOLDS = (64, 1024, 4096)  # the rows whose rings straddle a word, the front kernel's thread count, a wave of row words
CHORD_UNITS, WEAK_UNITS = 100, 1  # the distance (in 2^-10) two edges of a ring share: the largest, the smallest; every other one is 2 .. 64
SPAN = 200                     # seeded forward edges are shorter than this


def pair_id(n: int, i, j) -> np.ndarray:
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return i * (2 * int(n) - i - 1) // 2 + j - i - 1


def stepped_ids(n: int, centres) -> np.ndarray:
    ids = 8 + np.arange(n, dtype=np.int64)
    for centre in sorted(centres):
        ids[centre:] += 10 ** len(str(int(ids[centre - 1])))  # one digit more from the centre on
    return ids


def build(n: int, winner, loser, practical, *, units=None, nonviable=None, ids=None, seed: int = 1) -> dict:
    """``dominance_cases.build`` on arrays: edge ``e`` is ``winner[e]`` over ``loser[e]``, practical or statistical, at most one per unordered
    pair; ``units[e]`` a practical edge's distance beyond the threshold in 2^-10 (0: seeded, 2 .. 64); ``nonviable`` = (a, b) arrays of
    unresolved pairs without a test."""
    rng = np.random.default_rng(seed)
    n = int(n)
    winner, loser, practical = np.asarray(winner, dtype=np.int64), np.asarray(loser, dtype=np.int64), np.asarray(practical, dtype=bool)
    n_pairs = n * (n - 1) // 2
    cls = np.full(n_pairs, 5, dtype=np.uint8)
    jitter = rng.integers(-8, 9, size=n_pairs, dtype=np.int8) / 1024.0
    low, high = -0.01 + jitter, 0.0125 + jitter
    del jitter
    a, b = np.minimum(winner, loser), np.maximum(winner, loser)
    if len(a) and (a.min() < 0 or b.max() >= n or (a == b).any()):
        raise ValueError("an edge names a row outside the table, or a row twice")
    p = pair_id(n, a, b)
    if len(np.unique(p)) != len(p):
        raise ValueError("two edges for one pair")
    a_wins = winner == a
    units = np.zeros(len(p), dtype=np.int64) if units is None else np.asarray(units, dtype=np.int64)
    units = np.where(units > 0, units, rng.integers(2, 65, size=len(p)))
    inner = DELTA + units / 1024.0  # the bound on the winner's side
    cls[p] = np.where(practical, np.where(a_wins, 0, 1), np.where(a_wins, 2, 3))
    low[p] = np.where(practical, np.where(a_wins, inner, -inner - 0.03125), np.where(a_wins, 0.0078125, -0.046875))
    high[p] = np.where(practical, np.where(a_wins, inner + 0.03125, -inner), np.where(a_wins, 0.046875, -0.0078125))
    rate = 0.5 + 0.5 * (low + high)
    if nonviable is not None:
        q = pair_id(n, np.minimum(*nonviable), np.maximum(*nonviable))
        if (cls[q] != 5).any():
            raise ValueError("a pair has an edge and no test")
        cls[q] = 6
        low[q] = high[q] = rate[q] = np.nan
    ids = 8 + np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    return {"n": n, "ids": ids, "cls": cls, "low": low, "high": high, "rate": rate, "delta": DELTA, "edges": (winner, loser, practical)}


def edges_of_classes(n: int, cls) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The edge list of a case that has none (``dominance_cases``): from its classes, with the package's own unranking."""
    from farkle_ii_amd import round_robin as rr

    _, i, j = rr.pair_ids(n)
    cls = np.asarray(cls)
    e = np.flatnonzero(cls < 4)
    odd = (cls[e] & 1) == 1
    return np.where(odd, j[e], i[e]), np.where(odd, i[e], j[e]), cls[e] < 2


# ---- the sparse design: a path, rings on the thresholds, seeded forward edges, pairs without a test ----
def ring_centres(n: int, wanted=THRESHOLDS, last: bool = True) -> list[int]:
    """The centres of the rings of an ``n``-row design: every threshold whose ring fits below the last ring, and the ring that ends at
    row n - 1."""
    half = RING // 2
    end = n - RING if last else n
    return [t for t in wanted if t + half < end] + ([n - 1 - half] if last else [])


def _sparse_design(n: int, rng, centres, reserved=None):
    """``(winner, loser, practical, units, nonviable)``.  ``reserved`` = (lo, hi): no designed or seeded pair has both rows in [lo, hi)."""
    half = RING // 2
    ring_of = np.full(n, -1, dtype=np.int64)
    for k, c in enumerate(centres):
        ring_of[c - half:c + half + 1] = k
    band = np.zeros(n, dtype=bool) if reserved is None else (np.arange(n) >= reserved[0]) & (np.arange(n) < reserved[1])
    w, l, pr, un = [], [], [], []

    def add(a, b, practical, units=0):
        w.append(a), l.append(b), pr.append(practical), un.append(units)

    for i in range(n - 1):  # the path; inside a ring its edges are the ring's, all practical
        if band[i] and band[i + 1]:
            continue
        inside = ring_of[i] >= 0 and ring_of[i] == ring_of[i + 1]
        add(i, i + 1, inside or i % 3 != 0)
    for c in centres:
        lo, hi = c - half, c + half
        add(hi, lo, True)                 # closes the ring
        add(lo, c, True, CHORD_UNITS)     # the chord: lo -> c -> .. -> hi -> lo is a cycle of 6, the rows between keep 9
        if lo >= 130:                     # into the ring from earlier rows: rows of other threads of the front kernel lower its in-degree
            for source, target in ((lo - 24, c), (lo - 124, lo + 2), (lo - 23, lo), (lo - 14, hi)):
                add(source, target, source % 2 == 0)
    w, l, pr, un = (np.array(v, dtype=np.int64) for v in (w, l, pr, un))
    pr = pr.astype(bool)
    for c in centres:                     # the chord's twin, and two equally weak edges: ties across the centre
        lo = c - half
        un[(w == c) & (l == c + 1)] = CHORD_UNITS
        un[((w == lo + 1) & (l == lo + 2)) | ((w == c + 1) & (l == c + 2))] = WEAK_UNITS
    taken = pair_id(n, np.minimum(w, l), np.maximum(w, l))
    # ~12 n forward edges of span 2 .. SPAN - 1, none inside a ring, none twice
    i = rng.integers(0, n - 2, size=13 * n)
    j = i + rng.integers(2, SPAN, size=len(i))
    keep = j < n
    i, j = i[keep], j[keep]
    keep = ~((ring_of[i] >= 0) & (ring_of[i] == ring_of[j])) & ~(band[i] & band[j])
    i, j = i[keep], j[keep]
    p, first = np.unique(pair_id(n, i, j), return_index=True)
    first = np.sort(first[~np.isin(p, taken)])
    i, j = i[first], j[first]
    w, l = np.concatenate((w, i)), np.concatenate((l, j))
    pr, un = np.concatenate((pr, rng.random(len(i)) < 0.5)), np.concatenate((un, np.zeros(len(i), dtype=np.int64)))
    taken = pair_id(n, np.minimum(w, l), np.maximum(w, l))
    # ~n unresolved pairs without a test, anywhere in the table
    a, b = rng.integers(0, n, size=n + n // 8), rng.integers(0, n, size=n + n // 8)
    keep = (a != b) & ~(band[a] & band[b])
    a, b = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    q, first = np.unique(pair_id(n, a, b), return_index=True)
    first = first[~np.isin(q, taken)]
    return w, l, pr, un, (a[first], b[first])


def thresholds(n: int) -> dict:
    rng = np.random.default_rng(5000 + n)
    centres = ring_centres(n)
    w, l, pr, un, nonviable = _sparse_design(n, rng, centres)
    return build(n, w, l, pr, units=un, nonviable=nonviable, ids=stepped_ids(n, centres), seed=n)


BAND = (4000, 4160)  # words 62 - 64 of a row, both waves of the cycle workgroup


def dense_band_4160() -> dict:
    """The sparse design at n = 4 160 (rings on 64 and 1024), and among the rows of ``BAND`` nine pairs in ten directed, either way."""
    n = 4160
    rng = np.random.default_rng(4160)
    centres = ring_centres(n, wanted=(64, 1024), last=False)
    w, l, pr, un, nonviable = _sparse_design(n, rng, centres, reserved=BAND)
    i, j = np.triu_indices(BAND[1] - BAND[0], k=1)
    keep = rng.random(len(i)) < 0.9
    i, j = i[keep] + BAND[0], j[keep] + BAND[0]
    forward = rng.random(len(i)) < 0.5
    w, l = np.concatenate((w, np.where(forward, i, j))), np.concatenate((l, np.where(forward, j, i)))
    pr, un = np.concatenate((pr, rng.random(len(i)) < 0.5)), np.concatenate((un, np.zeros(len(i), dtype=np.int64)))
    return build(n, w, l, pr, units=un, nonviable=nonviable, ids=stepped_ids(n, centres), seed=n)


def ring_4160() -> dict:
    """One practical ring over all rows: component 0 of size n, cycle length n, front 1, one win and one loss a row."""
    n = 4160
    i = np.arange(n)
    return build(n, i, (i + 1) % n, np.ones(n, dtype=bool), seed=4161)


def total_order(n: int) -> dict:
    """Row i beats row j for all i < j, kinds as ``total_order_100``."""
    i, j = np.triu_indices(n, k=1)
    return build(n, i, j, (i + j) % 3 != 0, seed=n)


def dense(n: int, seed: int) -> dict:
    """``dense_random``'s law: nine pairs in ten directed, either way, either kind."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n, k=1)
    keep = rng.random(len(i)) < 0.9
    i, j = i[keep], j[keep]
    forward = rng.random(len(i)) < 0.5
    return build(n, np.where(forward, i, j), np.where(forward, j, i), rng.random(len(i)) < 0.5, seed=seed)


THRESHOLD_SIZES = (1024, 1025, 4096, 4097, 8192)
SIZE_CASES = {
    **{f"thresholds_{n}": functools.partial(thresholds, n) for n in THRESHOLD_SIZES},
    "dense_band_4160": dense_band_4160,
    "ring_4160": ring_4160,
    "total_order_1100": functools.partial(total_order, 1100),
    "dense_1100": functools.partial(dense, 1100, 1300),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    c = SIZE_CASES[name]()
    for key in ("ids", "cls", "low", "high", "rate"):
        c[key].setflags(write=False)
    return c


# ---- what the device is compared with ----
def ring_structure(n: int) -> dict:
    """One ring over all rows: component 0 of size n, front 1, every shortest cycle the ring itself, one win and one loss a row."""
    ones = np.ones(n, dtype=np.int64)
    return {"component": 0 * ones, "component_size": n * ones, "front": ones, "cycle_length": n * ones, "wins": ones, "losses": ones}


@functools.lru_cache(maxsize=None)
def expected(name: str) -> dict:
    """The sparse oracle's arrays of a size case under the rank of its ids, computed once.  ``ring_4160`` takes its components, fronts and
    cycle lengths from the closed form (both graphs are the ring: a search per member would cost n^2 steps) and only the extremes, the
    rates and the bits from the oracle."""
    import dominance_sparse_oracle as oracle

    c = case(name)
    return oracle.of_case(c, structures=[ring_structure(c["n"])] * 2 if name == "ring_4160" else None)
