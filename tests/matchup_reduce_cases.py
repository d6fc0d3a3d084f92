"""Synthetic records that drive ``fk_matchup_reduce`` to its edges, and a literal statement of its rule (test helper, not a conftest).

The entry takes host arrays (digest, sorted seat tuple, ``n_rounds``), so every regime of the reduce can be reached without a game
kernel: tuples that share a digest (the collision split, and ties on the 64-bit priority, which is a bijection of the digest), group
lengths at the strides of ``fkm_group_sums``, counts on both sides of every histogram bin edge, every seat count the entry accepts.

``literal_reduce`` restates the rule of ``analysis/rng_diagnostics.py`` as the reference states it — a dict of groups in record order,
Python ints, one loop per (group, lag) — and shares no structure with ``rng_matchups.host_reduce`` (``np.unique``, stable argsort,
prefix sums) or with the device code (radix sorts, segment scans, one wave per group).  Its only import from the project is
``rng_matchups.priority``.

Every builder is seeded and returns ``(records, k, lags, caps)``.  The digest is a function of the tuple (drawn per tuple; several
tuples may share one), and the records are interleaved by a seeded permutation, so grouping has to bring every group together again.

Two points of the entry bound what a case can ask: a lag is at most 65 535 (``check_lags``), so the group that holds every record
(200 000 of them) takes lags ``(1, 65 534, 65 535)`` and a group of 65 536 records stands beside it, in which the largest lag leaves
exactly one pair; and ``M = cap + ties``, so a variant of ``tie_batches`` with 0 or 1 tied groups behind the cut cannot overflow the
binding's slack of 64 — the replay with a larger ``out_capacity`` runs in the variants with 4 095 ties and more."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from farkle_ii_amd import rng_matchups as rm

U64_MAX = (1 << 64) - 1
ROUNDS_MAX = 0x7FFF
SEAT_MAX = 65_533            # the largest table index of a 65 534-strategy table
TIE_BATCH = 4096             # entries the cap's tie extension reads per host round trip (fk_matchup_reduce)
REPLAY_SLACK = 64            # Backend.matchup_reduce's first out_capacity is cap + 64


# ------------------------------------------------------------------------------------------------------- the literal reference
def literal_bin(count: int, minimum: int) -> int:
    """``_observation_histogram_bin``: the count itself (at most 32 767) below the minimum, then one bin per power of two."""
    if count < minimum:
        return min(count, 32767)
    return minimum + (count - minimum + 1).bit_length() - 1


def literal_reduce(records: dict, k: int, lags, cap) -> tuple[dict, dict]:
    """``(summary, kept)``: the counts, the histogram ``{bin: groups}`` and the eligible groups' priorities in ascending order; the
    kept groups ``{tuple: (digest, count, [[pairs, sum x, sum y, sum x^2, sum y^2, sum xy] per lag])}``."""
    lags = [int(v) for v in lags]
    digests = np.asarray(records["digest"], dtype=np.uint64).tolist()
    tuples = np.asarray(records["seats"], dtype=np.uint16).reshape(-1, k).tolist()
    rounds = np.asarray(records["rounds"], dtype=np.uint16).tolist()
    groups: dict[tuple, tuple[int, list[int]]] = {}
    for d, t, r in zip(digests, tuples, rounds):
        key = tuple(t)
        if key in groups:
            assert groups[key][0] == d, "the digest is a function of the tuple"
            groups[key][1].append(r)
        else:
            groups[key] = (d, [r])
    minimum = min(lags) + 2
    histogram: dict[int, int] = {}
    eligible = []
    for key, (d, series) in groups.items():
        b = literal_bin(len(series), minimum)
        histogram[b] = histogram.get(b, 0) + 1
        if len(series) >= minimum:
            eligible.append(key)
    prio = rm.priority(np.array([groups[key][0] for key in eligible], dtype=np.uint64), k).tolist() if eligible else []
    ranked = sorted(zip(prio, eligible), key=lambda pe: pe[0])
    E = M = len(ranked)
    cut = cap is not None and 0 < cap < E
    if cut:
        M = cap
        while M < E and ranked[M][0] == ranked[cap - 1][0]:  # every group tied with the last one kept
            M += 1
    kept = {}
    for _, key in ranked[:M]:
        d, series = groups[key]
        sums = []
        for lag in lags:
            pairs = sx = sy = sxx = syy = sxy = 0
            for i in range(lag, len(series)):
                x, y = series[i - lag], series[i]
                pairs += 1
                sx += x
                sy += y
                sxx += x * x
                syy += y * y
                sxy += x * y
            sums.append([pairs, sx, sy, sxx, syy, sxy])
        kept[key] = (d, len(series), sums)
    summary = {"observations": len(digests), "candidate_groups": len(groups), "eligible_groups": E, "selected_groups": M,
               "tied_behind_cut": M - cap if cut else 0, "minimum": minimum,
               "histogram": histogram, "priorities": [p for p, _ in ranked], "counts": sorted(len(s) for _, s in groups.values())}
    return summary, kept


def histogram_array(summary: dict) -> np.ndarray:
    """The histogram in the entry's layout: ``[minimum + 64]`` groups per bin code."""
    out = np.zeros(summary["minimum"] + 64, dtype=np.uint64)
    for b, c in summary["histogram"].items():
        out[b] = c
    return out


def kept_groups(result: dict) -> dict:
    """A reduce result (device or host) keyed like ``literal_reduce``'s second value."""
    k = int(result["k"])
    seats = np.asarray(result["seats"]).reshape(-1, k).tolist()
    out = {tuple(t): (int(d), int(c), s) for t, d, c, s in zip(seats, np.asarray(result["digest"], dtype=np.uint64).tolist(),
                                                                np.asarray(result["count"]).tolist(), np.asarray(result["sums"]).tolist())}
    assert len(out) == len(seats), "a tuple was returned twice"
    return out


def tied_runs(priorities: list[int]) -> list[tuple[int, int]]:
    """``[begin, end)`` of every run of at least two equal values of an ascending list."""
    runs, s = [], 0
    for i in range(1, len(priorities) + 1):
        if i == len(priorities) or priorities[i] != priorities[s]:
            if i - s >= 2:
                runs.append((s, i))
            s = i
    return runs


# ------------------------------------------------------------------------------------------------------- building blocks
def _tuples(rng, n: int, k: int, lo: int = 2, hi: int = SEAT_MAX - 2) -> np.ndarray:
    """``n`` different strictly ascending tuples with entries in ``[lo, hi]`` (a game seats a strategy once)."""
    rows = np.sort(rng.integers(lo, hi - k + 2, size=(n + n // 4 + 8, k)), axis=1) + np.arange(k)
    rows = np.unique(rows, axis=0)
    assert len(rows) >= n
    return rows[rng.permutation(len(rows))[:n]].astype(np.int64)


def _digests(rng, n: int) -> list[int]:
    out = np.unique(rng.integers(1 << 8, U64_MAX - (1 << 8), size=n + 8, dtype=np.uint64))
    return rng.permutation(out)[:n].tolist()


def _assemble(keys, digests, counts, k: int, rng, round_values=None) -> dict:
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, k)
    assert keys.min() >= 0 and keys.max() <= SEAT_MAX and len(np.unique(keys, axis=0)) == len(keys) == len(digests) == len(counts)
    owner = np.repeat(np.arange(len(keys)), np.asarray(counts, dtype=np.int64))
    owner = owner[rng.permutation(len(owner))]
    if round_values is None:
        rounds = rng.integers(0, ROUNDS_MAX + 1, size=len(owner))
    else:
        rounds = rng.choice(np.asarray(round_values), size=len(owner))
    return {"digest": np.array(digests, dtype=np.uint64)[owner], "seats": keys[owner].astype(np.uint16), "rounds": rounds.astype(np.uint16)}


# ------------------------------------------------------------------------------------------------------- the cases
STRIDE_LAGS = (1, 2, 63, 64, 65, 128, 200)
STRIDE_LENGTHS = (1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 264, 265)


def strides():
    """One wave strides a group 64 positions at a time from ``lag + lane``: lengths, and lengths minus a lag, at 63 .. 65 and
    127 .. 129, eligible groups shorter than the larger lags, ``n_rounds`` at its least and greatest value."""
    rng = np.random.default_rng(11)
    n = len(STRIDE_LENGTHS)
    return _assemble(_tuples(rng, n, 2), _digests(rng, n), STRIDE_LENGTHS, 2, rng, (0, 1, 17, ROUNDS_MAX)), 2, STRIDE_LAGS, (None, 4)


def every_k(k: int):
    """About 300 tuples of 1 .. 8 records, with pairs of tuples that differ only in column 0 or only in column k - 1; the two tuples
    of a pair share a digest, so the collision split runs its k + 1 passes at this k.  Indices 0 and 65 533 appear."""
    rng = np.random.default_rng(1000 + k)
    n_pairs = 1 if k == 1 else 3
    base = _tuples(rng, 300 + 2 * n_pairs, k)
    keys, digests, counts = [base[2 * n_pairs:]], _digests(rng, 300), rng.integers(1, 9, size=300).tolist()
    pair_digests = _digests(np.random.default_rng(2000 + k), 2 * n_pairs)
    pair_counts = ((4, 5), (2, 6), (3, 3))
    for i in range(n_pairs):
        for side, (col, values, b) in enumerate(((0, (0, 1), base[i]), (k - 1, (SEAT_MAX - 1, SEAT_MAX), base[n_pairs + i]))):
            for v, c in zip(values, pair_counts[i]):
                t = b.copy()
                t[col] = v
                keys.append(t[None, :])
                digests.append(pair_digests[2 * i + side])
                counts.append(c)
    return _assemble(np.concatenate(keys), digests, counts, k, rng), k, (1, 3), (None, 50)


def collisions(k: int):
    """Runs of 2 .. 40 tuples on one digest each, eligible and ineligible counts mixed inside a run; the tuples of a run differ only
    in their last or only in their first column.  Adjacent digests d, d + 1 and the digests 0 and 2^64 - 1.  The caps sit around the
    first and the longest run of tied priorities and around the number of eligible groups."""
    rng = np.random.default_rng(300 + k)
    lags = (1, 2)
    d, r1, r2, r3 = _digests(rng, 4)
    runs = ((r1, 2), (r2, 3), (d, 7), (d + 1, 12), (0, 5), (U64_MAX, 40), (r3, 9))
    keys, digests, counts = [], [], []
    bases_last, bases_first = _tuples(rng, len(runs), k, hi=SEAT_MAX - 40), _tuples(rng, len(runs), k, lo=100)
    for i, (dig, size) in enumerate(runs):
        n_last = (size + 1) // 2 if size >= 4 else size
        for j in range(size):
            t = (bases_last if j < n_last else bases_first)[i].copy()
            if j < n_last:
                t[k - 1] = SEAT_MAX - j          # (the base ends below SEAT_MAX - 40)
            else:
                t[0] = j - n_last                # (the base starts at 100 or above)
            keys.append(t[None, :])
            digests.append(dig)
        c = rng.integers(1, 10, size=size)
        c[0], c[1] = 2, 5                         # one group below the minimum of 3 and one above it in every run
        counts.extend(c.tolist())
    n_plain = 150
    keys.append(_tuples(rng, n_plain, k, lo=200, hi=SEAT_MAX - 100))
    digests.extend(_digests(rng, n_plain))
    counts.extend(rng.integers(1, 10, size=n_plain).tolist())
    records = _assemble(np.concatenate(keys), digests, counts, k, rng)
    summary, _ = literal_reduce(records, k, lags, None)
    E, tied = summary["eligible_groups"], tied_runs(summary["priorities"])
    caps = {E - 1, E, E + 1}
    for s, e in (tied[0], max(tied, key=lambda se: se[1] - se[0])):
        caps |= {s, s + 1, s + (e - s) // 2 + 1, e - 1, e}  # before the run; its first, a middle, its last-but-one member; its end
    return records, k, lags, (None,) + tuple(sorted(c for c in caps if c > 0))


TIE_VARIANTS = (0, 1, TIE_BATCH - 1, TIE_BATCH, TIE_BATCH + 1, "end")
TIE_KEPT_OF_RUN = 5   # members of the tied run in front of the cut
TIE_END_GROUPS = 5000


def tie_batches(variant):
    """Tied eligible groups of 3 records each on one digest beside 300 ordinary groups; the cap keeps five of the tied run, so
    ``variant`` groups follow the cut (0, 1, one batch less one, one batch, one batch and one), or the run of 5 000 ends the
    eligible list (``"end"``: the extension stops because ``M`` reaches ``E``)."""
    rng = np.random.default_rng(700 + TIE_VARIANTS.index(variant))
    k, lags, n_plain = 3, (1,), 300
    n_tied = TIE_END_GROUPS if variant == "end" else variant + TIE_KEPT_OF_RUN
    pool = _digests(rng, n_plain + 1)
    order = np.argsort(rm.priority(np.array(pool, dtype=np.uint64), k), kind="stable").tolist()
    tied_digest = pool[order[-1] if variant == "end" else order[len(order) // 2]]  # greatest priority / the median
    plain = [p for p in pool if p != tied_digest]
    keys = _tuples(rng, n_plain + n_tied, k)
    counts = rng.integers(1, 7, size=n_plain).tolist() + [3] * n_tied
    records = _assemble(keys, plain + [tied_digest] * n_tied, counts, k, rng)
    summary, _ = literal_reduce(records, k, lags, None)
    (s, e), = tied_runs(summary["priorities"])
    assert e - s == n_tied
    return records, k, lags, (s + TIE_KEPT_OF_RUN,)


BIN_EDGE_POWERS = tuple(range(13))


def bins_edges():
    """Minimum 3: counts below it, and both sides of every bin edge ``3 + 2^j - 1`` up to j = 12."""
    rng = np.random.default_rng(41)
    counts = [1, 2, 3, 4, 5, 9, 10, 17, 18, 33, 34]
    for j in BIN_EDGE_POWERS:
        counts += [3 + (1 << j) - 2, 3 + (1 << j) - 1]
    return _assemble(_tuples(rng, len(counts), 2), _digests(rng, len(counts)), counts, 2, rng), 2, (1,), (None, 3)


def bins_clamp():
    """Minimum 40 002: groups of 32 766 .. 35 000 records are below it, the last two in the clamped bin 32 767; nothing is eligible."""
    rng = np.random.default_rng(42)
    counts = [32766, 32767, 32768, 35000]
    return _assemble(_tuples(rng, 4, 2), _digests(rng, 4), counts, 2, rng), 2, (40000,), (None, 10)


def one_record():
    rng = np.random.default_rng(51)
    return _assemble(_tuples(rng, 1, 2), _digests(rng, 1), [1], 2, rng), 2, (1,), (None, 1)


def one_group():
    """Every record in one group at k = 1, all at the greatest ``n_rounds``: the largest sum is 2^30 x 2 x 10^5."""
    rng = np.random.default_rng(52)
    return _assemble([[SEAT_MAX]], _digests(rng, 1), [200_000], 1, rng, (ROUNDS_MAX,)), 1, (1, 65_534, 65_535), (None, 1)


def one_group_at_the_largest_lag():
    """65 536 records in one group: the largest lag the entry accepts leaves one pair."""
    rng = np.random.default_rng(53)
    return _assemble([[0]], _digests(rng, 1), [65_536], 1, rng), 1, (1, 65_534, 65_535), (None,)


def singletons():
    rng = np.random.default_rng(54)
    n = 70_000
    return _assemble(_tuples(rng, n, 2), _digests(rng, n), [1] * n, 2, rng), 2, (1,), (None, 5)


BUILDERS = {"strides": strides, "bins_edges": bins_edges, "bins_clamp": bins_clamp, "one_record": one_record, "one_group": one_group,
            "one_group_at_the_largest_lag": one_group_at_the_largest_lag, "singletons": singletons}
BUILDERS.update({f"every_k_{k}": (lambda k=k: every_k(k)) for k in range(1, 17)})
BUILDERS.update({f"collisions_{k}": (lambda k=k: collisions(k)) for k in (3, 16)})
BUILDERS.update({f"tie_batches_{v}": (lambda v=v: tie_batches(v)) for v in TIE_VARIANTS})
NAMES = tuple(BUILDERS)


@lru_cache(maxsize=None)
def case(name: str):
    """``(records, k, lags, caps)`` of a named case, built once per process and left unchanged."""
    records, k, lags, caps = BUILDERS[name]()
    for a in records.values():
        a.setflags(write=False)
    return records, k, tuple(lags), tuple(caps)


@lru_cache(maxsize=None)
def literal(name: str, cap):
    records, k, lags, _ = case(name)
    return literal_reduce(records, k, lags, cap)
