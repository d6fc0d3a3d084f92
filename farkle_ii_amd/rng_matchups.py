"""Lag autocorrelation rows of the reference's RNG diagnostics, MATCHUP family, and the group-selection report.

``analysis/rng_diagnostics.py`` keys every game by its seat strategy IDs sorted ascending and padded with -1 to ``max_players``
columns (``_extract_batch_arrays`` :1092-1150); the group's ``group_id`` is ``blake2b(int32 LE [k, ids..., -1...], digest_size=8,
person=b"farkle-m")`` read little-endian (``_matchup_ids`` :1173-1185), but groups are the FULL identity ``(group_type, k,
group_id, p0 ... p{max_players-1})``.  A group's series is ``n_rounds`` ordered by ``(root_seed, k, shuffle_index, game_index)``;
per lag ``_OnlineMetric`` (:2032-2076) takes the six sums over pairs (position i - lag, position i).

A group is eligible when its count is at least ``min(lags) + 2`` (run :592).  Eligible matchup groups are ranked across every k
of the root by ``(priority, group_type, k, group_id, p0 ...)`` with ``_priority`` (:1281) and the first
``analysis.rng_max_matchup_groups`` are kept (``_effective_max_matchup_groups`` :978, ``_write_or_reuse_selection``
:1577-1800); strategy groups are selected whenever eligible.  Since the cap spans player counts, a per-k pass hands up only its
own top-``cap`` eligible groups (:class:`MatchupGroups`): the root's top-``cap`` is a subset of their union.

Per game this family needs a digest, the sorted seat tuple and ``n_rounds`` (``fk_tournament_run_matchups``); the grouped
reduce is ``fk_matchup_reduce`` on the device.  This module is the host statement of the same rule (NumPy) and the merge of
per-k results into the root-level rows (``_stats_schema``, ``_rows_for_online_group`` :2110-2160) and report (:1664-1701)."""
from __future__ import annotations

import hashlib
import json
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

from .rng_lags import STATS_NOTE, autocorr

GROUP_STRATEGY, GROUP_MATCHUP = 0, 1
DEFAULT_MAX_MATCHUP_GROUPS = 100_000  # _DEFAULT_MAX_MATCHUP_GROUPS
METHOD_VERSION = 4                    # _DIAGNOSTIC_METHOD_VERSION
MATCHUP_ORDER = "root_seed,k,shuffle_index,game_index"  # ",".join(_GAME_COORDINATE_COLUMNS)
SUM_COLS = 6  # pairs, sum x, sum y, sum x^2, sum y^2, sum xy
PERSON = b"farkle-m"


def effective_cap(configured: int | None) -> int | None:
    """``_effective_max_matchup_groups`` (:978): default 100 000, a value <= 0 means no cap."""
    if configured is None:
        return DEFAULT_MAX_MATCHUP_GROUPS
    return int(configured) if int(configured) > 0 else None


def minimum_observations(lags: Sequence[int]) -> int:
    return min(int(v) for v in lags) + 2


# ---------------------------------------------------------------------------------------------------------------- digest
def digest_hashlib(k: int, sorted_ids: Sequence[int], max_players: int) -> int:
    """The reference's digest of one tuple, with ``hashlib``."""
    words = [int(k), *(int(v) for v in sorted_ids)] + [-1] * (max_players - len(sorted_ids))
    raw = np.asarray(words, dtype="<i4").tobytes()
    return int.from_bytes(hashlib.blake2b(raw, digest_size=8, person=PERSON).digest(), "little")


_IV = np.array([0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
                0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179], dtype=np.uint64)
_SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
          (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
          (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
          (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
          (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))


def _rotr(x: np.ndarray, n: int) -> np.ndarray:
    return (x >> np.uint64(n)) | (x << np.uint64(64 - n))


def digests(k: int, sorted_ids: np.ndarray, max_players: int) -> np.ndarray:
    """Vectorised restatement of the digest: ONE BLAKE2b compression per tuple (the message is 4 (1 + max_players) <= 128
    bytes), parameter word 0x01010008, ``person`` XORed into h[6], digest = h0 ^ v0 ^ v8 after twelve rounds."""
    ids = np.asarray(sorted_ids, dtype=np.int32).reshape(-1, k)
    n = len(ids)
    if 4 * (1 + max_players) > 128 or max_players < k:
        raise ValueError("max_players must be in [k, 31]")
    w = np.zeros((n, 32), dtype=np.uint64)
    w[:, 0] = k
    w[:, 1:k + 1] = ids.view(np.uint32)
    w[:, k + 1:max_players + 1] = 0xFFFFFFFF
    m = [w[:, 2 * i] | (w[:, 2 * i + 1] << np.uint64(32)) for i in range(16)]
    h0 = _IV[0] ^ np.uint64(0x01010008)
    v = [np.full(n, h0, dtype=np.uint64)] + [np.full(n, x, dtype=np.uint64) for x in _IV[1:]] + [np.full(n, x, dtype=np.uint64) for x in _IV]
    v[6] ^= np.uint64(int.from_bytes(PERSON, "little"))
    v[12] ^= np.uint64(4 * (1 + max_players))
    v[14] = ~v[14]

    def g(a, b, c, d, x, y):
        v[a] = v[a] + v[b] + x
        v[d] = _rotr(v[d] ^ v[a], 32)
        v[c] = v[c] + v[d]
        v[b] = _rotr(v[b] ^ v[c], 24)
        v[a] = v[a] + v[b] + y
        v[d] = _rotr(v[d] ^ v[a], 16)
        v[c] = v[c] + v[d]
        v[b] = _rotr(v[b] ^ v[c], 63)

    with np.errstate(over="ignore"):
        for r in range(12):
            s = _SIGMA[r % 10]
            g(0, 4, 8, 12, m[s[0]], m[s[1]])
            g(1, 5, 9, 13, m[s[2]], m[s[3]])
            g(2, 6, 10, 14, m[s[4]], m[s[5]])
            g(3, 7, 11, 15, m[s[6]], m[s[7]])
            g(0, 5, 10, 15, m[s[8]], m[s[9]])
            g(1, 6, 11, 12, m[s[10]], m[s[11]])
            g(2, 7, 8, 13, m[s[12]], m[s[13]])
            g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return np.uint64(h0) ^ v[0] ^ v[8]


def splitmix64(values: np.ndarray) -> np.ndarray:
    """``_splitmix64`` (:1258)."""
    with np.errstate(over="ignore"):
        x = np.asarray(values, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def priority(group_id: np.ndarray, k: np.ndarray | int, group_type: int = GROUP_MATCHUP) -> np.ndarray:
    """``_priority`` (:1281): splitmix64(group_id ^ k << 48 ^ group_type << 63 ^ 0xD1B54A32D192ED03)."""
    v = np.asarray(group_id, dtype=np.uint64) ^ (np.asarray(k, dtype=np.uint64) << np.uint64(48))
    v = v ^ (np.uint64(group_type) << np.uint64(63))
    return splitmix64(v ^ np.uint64(0xD1B54A32D192ED03))


def histogram_bin(counts: np.ndarray, minimum: int) -> np.ndarray:
    """``_observation_histogram_bin`` (:1568)."""
    counts = np.asarray(counts, dtype=np.int64)
    out = np.zeros(counts.size, dtype=np.int64)
    below = counts < minimum
    out[below] = np.minimum(counts[below], 32767)
    if np.any(~below):
        out[~below] = minimum + np.floor(np.log2(counts[~below] - minimum + 1)).astype(np.int64)
    return out


def histogram_label(code: int, minimum: int) -> str:
    """``_histogram_label`` (:1803)."""
    if code < minimum:
        return str(code)
    power = code - minimum
    return f"{minimum + (1 << power) - 1}-{minimum + (1 << (power + 1)) - 2}"


# ---------------------------------------------------------------------------------------------------------------- records
def records_from_rows(rows: np.ndarray, strategy_ids: np.ndarray, k: int, max_players: int) -> dict:
    """The per-game records of ``fk_tournament_run_matchups`` from engine rows (AoS, coordinate order): digest, the seats' table
    indices in ascending-ID order, n_rounds (15 bits)."""
    ids = np.asarray(strategy_ids, dtype=np.int32)
    idx = rows["seats"]["strategy"].astype(np.int64).reshape(len(rows), k)
    sid = ids[idx]
    order = np.lexsort((idx, sid), axis=1) if k > 1 else np.zeros_like(idx)
    idx = np.take_along_axis(idx, order, axis=1)
    sid = np.take_along_axis(sid, order, axis=1)
    return {"digest": digests(k, sid, max_players) if len(rows) else np.zeros(0, dtype=np.uint64),
            "seats": idx.astype(np.uint16), "rounds": (rows["n_rounds"] & 0x7FFF).astype(np.uint16)}


def concat_records(parts: Sequence[dict], k: int) -> dict:
    """Records of contiguous ranges in range order -> the records of their union."""
    parts = list(parts)
    if not parts:
        return {"digest": np.zeros(0, dtype=np.uint64), "seats": np.zeros((0, k), dtype=np.uint16), "rounds": np.zeros(0, dtype=np.uint16)}
    return {"digest": np.concatenate([p["digest"] for p in parts]),
            "seats": np.concatenate([np.asarray(p["seats"]).reshape(-1, k) for p in parts]),
            "rounds": np.concatenate([p["rounds"] for p in parts])}


def host_reduce(records: dict, k: int, lags: Sequence[int], cap: int | None) -> dict:
    """Host statement of ``fk_matchup_reduce`` (same result layout): groups = equal tuples, each in record order; the eligible
    groups in ascending 64-bit priority, cut after ``cap`` plus every group tied with the last one kept."""
    lags = tuple(int(v) for v in lags)
    minimum = minimum_observations(lags)
    seats = np.asarray(records["seats"], dtype=np.uint16).reshape(-1, k)
    digest = np.asarray(records["digest"], dtype=np.uint64)
    rounds = np.asarray(records["rounds"], dtype=np.int64)
    n = len(digest)
    hist = np.zeros(minimum + 64, dtype=np.uint64)
    empty = {"k": k, "lags": lags, "observations": n, "candidate_groups": 0, "eligible_groups": 0, "histogram": hist,
             "digest": np.zeros(0, dtype=np.uint64), "seats": np.zeros((0, k), dtype=np.uint16), "count": np.zeros(0, dtype=np.int64),
             "sums": np.zeros((0, len(lags), SUM_COLS), dtype=np.int64)}
    if n == 0:
        return empty
    _, inverse = np.unique(seats, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable")
    seg = inverse[order]
    starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    counts = np.diff(np.r_[starts, n])
    np.add.at(hist, histogram_bin(counts, minimum), 1)
    first = order[starts]
    prio = priority(digest[first], k)
    eligible = np.flatnonzero(counts >= minimum)
    sel = eligible[np.argsort(prio[eligible], kind="stable")]
    M = len(sel)
    if cap is not None and cap > 0 and len(sel) > cap:
        last = prio[sel[cap - 1]]
        M = cap + int(np.count_nonzero(prio[sel[cap:]] == last))  # (sorted: the ties follow the cut)
    sel = sel[:M]
    # per-group lag sums by prefix sums over the grouped order (exact int64)
    r = rounds[order]
    pos = np.arange(n) - np.repeat(starts, counts)
    sums = np.zeros((M, len(lags), SUM_COLS), dtype=np.int64)
    s_start, s_end = starts[sel], starts[sel] + counts[sel]
    for li, lag in enumerate(lags):
        valid = pos >= lag
        x = np.zeros(n, dtype=np.int64)
        if lag < n:
            x[lag:] = r[:n - lag]
        y = r
        for c, val in enumerate((np.ones(n, dtype=np.int64), x, y, x * x, y * y, x * y)):
            cs = np.r_[0, np.cumsum(np.where(valid, val, 0))]
            sums[:, li, c] = cs[s_end] - cs[s_start]
    out = dict(empty)
    out.update(candidate_groups=len(starts), eligible_groups=len(eligible), histogram=hist, digest=digest[first[sel]],
               seats=seats[first[sel]], count=counts[sel].astype(np.int64), sums=sums)
    return out


# ---------------------------------------------------------------------------------------------------------------- per-k groups
@dataclass
class MatchupGroups:
    """One (root, k): its counts and histogram, and its own top-``cap`` eligible matchup groups in priority-tuple order."""

    k: int
    lags: tuple[int, ...]
    max_players: int
    observations: int
    candidate_groups: int
    eligible_groups: int
    histogram: dict[int, int]            # bin code -> groups
    priority: np.ndarray                 # uint64 [G]
    group_id: np.ndarray                 # uint64 [G]
    participants: np.ndarray             # int32 [G][max_players], sorted IDs padded with -1
    count: np.ndarray                    # int64 [G]
    sums: np.ndarray                     # int64 [G][n_lags][6]
    extra: dict = field(default_factory=dict)

    @classmethod
    def from_reduce(cls, res: dict, strategy_ids: np.ndarray, max_players: int, cap: int | None) -> "MatchupGroups":
        """A reduce result (device or host) -> the exact top-``cap`` by the full tuple (ties on the 64-bit priority are broken here)."""
        k, lags = int(res["k"]), tuple(res["lags"])
        ids = np.asarray(strategy_ids, dtype=np.int32)
        seats = np.asarray(res["seats"]).reshape(-1, k)
        part = np.full((len(seats), max_players), -1, dtype=np.int32)
        part[:, :k] = ids[seats.astype(np.int64)]
        gid = np.asarray(res["digest"], dtype=np.uint64)
        prio = priority(gid, k)
        order = np.lexsort(tuple(part[:, j] for j in reversed(range(max_players))) + (gid, prio))
        if cap is not None and cap > 0:
            order = order[:cap]
        hist = {int(b): int(c) for b, c in enumerate(np.asarray(res["histogram"])) if c}
        return cls(k, lags, max_players, int(res["observations"]), int(res["candidate_groups"]), int(res["eligible_groups"]), hist,
                   prio[order], gid[order], part[order], np.asarray(res["count"], dtype=np.int64)[order],
                   np.asarray(res["sums"], dtype=np.int64)[order])

    def to_table(self):
        """``<k>p_rng_matchup_groups.parquet``: one row per kept group; counts and histogram in the schema metadata."""
        import pyarrow as pa

        cols: dict[str, Any] = {"n_players": pa.array(np.full(len(self.count), self.k, dtype=np.int16)),
                                "priority": pa.array(self.priority, type=pa.uint64()), "matchup_id": pa.array(self.group_id, type=pa.uint64())}
        for j in range(self.max_players):
            cols[f"p{j}"] = pa.array(self.participants[:, j], type=pa.int32())
        cols["observations"] = pa.array(self.count, type=pa.int64())
        for c, name in enumerate(("lagged_pairs", "n_rounds_sum_x", "n_rounds_sum_y", "n_rounds_sum_x2", "n_rounds_sum_y2", "n_rounds_sum_xy")):
            cols[name] = pa.array([list(map(int, row)) for row in self.sums[:, :, c]], type=pa.list_(pa.int64()))
        meta = {"k": self.k, "lags": list(self.lags), "max_players": self.max_players, "observations": self.observations,
                "candidate_groups": self.candidate_groups, "eligible_groups": self.eligible_groups,
                "histogram": {str(b): c for b, c in sorted(self.histogram.items())}, **self.extra}
        return pa.table(cols).replace_schema_metadata({b"farkle_rng_matchup_groups": json.dumps(meta, sort_keys=True).encode()})

    @classmethod
    def from_table(cls, table) -> "MatchupGroups":
        meta = json.loads(table.schema.metadata[b"farkle_rng_matchup_groups"])
        mp = int(meta["max_players"])
        n, nl = table.num_rows, len(meta["lags"])
        sums = np.zeros((n, nl, SUM_COLS), dtype=np.int64)
        for c, name in enumerate(("lagged_pairs", "n_rounds_sum_x", "n_rounds_sum_y", "n_rounds_sum_x2", "n_rounds_sum_y2", "n_rounds_sum_xy")):
            if n:
                sums[:, :, c] = np.asarray(table.column(name).to_pylist(), dtype=np.int64).reshape(n, nl)
        part = np.stack([table.column(f"p{j}").to_numpy() for j in range(mp)], axis=1).astype(np.int32) if n else np.zeros((0, mp), np.int32)
        extra = {key: v for key, v in meta.items() if key not in ("k", "lags", "max_players", "observations", "candidate_groups",
                                                                 "eligible_groups", "histogram")}
        return cls(int(meta["k"]), tuple(meta["lags"]), mp, int(meta["observations"]), int(meta["candidate_groups"]),
                   int(meta["eligible_groups"]), {int(b): int(c) for b, c in meta["histogram"].items()},
                   table.column("priority").to_numpy().astype(np.uint64), table.column("matchup_id").to_numpy().astype(np.uint64),
                   part, table.column("observations").to_numpy().astype(np.int64), sums, extra)


# ---------------------------------------------------------------------------------------------------------------- root level
@dataclass
class StrategyFamily:
    """The strategy groups of one k for the report: every strategy of the table has ``observations`` = shuffles of the root."""

    k: int
    n_strategies: int
    observations: int


def select(groups: Sequence[MatchupGroups], strategies: Sequence[StrategyFamily], lags: Sequence[int], cap: int | None,
           partition_count: int) -> tuple[list[dict[str, Any]], dict[str, Any]]:
    """Selection across every k of the root (``_write_or_reuse_selection``): the matchup rows of the selected groups (in group
    identity order) and the report."""
    lags = tuple(int(v) for v in lags)
    minimum = minimum_observations(lags)
    totals = {"strategy": 0, "matchup": 0}
    eligible = {"strategy": 0, "matchup": 0}
    histogram: dict[tuple[str, int], int] = {}
    for st in strategies:
        totals["strategy"] += st.n_strategies
        if st.observations >= minimum:
            eligible["strategy"] += st.n_strategies
        code = int(histogram_bin(np.array([st.observations]), minimum)[0])
        if st.n_strategies:
            histogram[("strategy", code)] = histogram.get(("strategy", code), 0) + st.n_strategies
    for g in groups:
        totals["matchup"] += g.candidate_groups
        eligible["matchup"] += g.eligible_groups
        for code, c in g.histogram.items():
            histogram[("matchup", code)] = histogram.get(("matchup", code), 0) + c
    # the union of the per-k lists, ranked by (priority, group_type, k, group_id, p0 ...)
    keys, owners = [], []
    for gi, g in enumerate(groups):
        for j in range(len(g.count)):
            keys.append((int(g.priority[j]), GROUP_MATCHUP, g.k, int(g.group_id[j]), *(int(v) for v in g.participants[j])))
            owners.append((gi, j))
    ranked = sorted(range(len(keys)), key=lambda i: keys[i])
    capped, cutoff = 0, None
    if cap is not None and eligible["matchup"] > cap:
        ranked = ranked[:cap]
        cutoff = list(keys[ranked[-1]])
        capped = eligible["matchup"] - cap
    kept = sorted(ranked, key=lambda i: keys[i][2:])  # identity order: k, group_id, participants
    rows: list[dict[str, Any]] = []
    for i in kept:
        g, j = groups[owners[i][0]], owners[i][1]
        rows.extend(matchup_rows(g.k, int(g.group_id[j]), g.participants[j], int(g.count[j]), g.sums[j], lags))
    below = totals["strategy"] + totals["matchup"] - eligible["strategy"] - eligible["matchup"]
    report: dict[str, Any] = {
        "selection_schema_version": 1,
        "method_version": METHOD_VERSION,
        "partition_count": int(partition_count),
        "minimum_usable_observations": minimum,
        "normalized_lags": list(lags),
        "effective_matchup_group_cap": cap,
        "total_candidate_groups": totals["strategy"] + totals["matchup"],
        "candidate_strategy_groups": totals["strategy"],
        "candidate_matchup_groups": totals["matchup"],
        "eligible_groups": eligible["strategy"] + eligible["matchup"],
        "eligible_strategy_groups": eligible["strategy"],
        "eligible_matchup_groups": eligible["matchup"],
        "selected_strategy_groups": eligible["strategy"],
        "selected_matchup_groups": eligible["matchup"] - capped,
        "below_minimum_observation_groups": below,
        "deterministically_capped_groups": capped,
        "exclusion_reasons": {"below_minimum_usable_observations": below, "deterministic_priority_cap": capped},
        "observation_count_distribution": [{"summary_level": label, "bin": histogram_label(code, minimum), "groups": c}
                                           for (label, code), c in sorted(histogram.items())],
        "priority_cutoff": cutoff,
        "completeness_status": "blocked_by_cap" if capped else "planned_complete",
    }
    report["selected_groups"] = int(report["selected_strategy_groups"]) + int(report["selected_matchup_groups"])
    return rows, report


def matchup_rows(k: int, group_id: int, participants: Sequence[int], count: int, sums: np.ndarray, lags: Sequence[int],
                 note: str = STATS_NOTE) -> list[dict[str, Any]]:
    """``_rows_for_online_group`` for one matchup group: one ``n_rounds`` row per lag (no win indicator)."""
    ids = [int(v) for v in participants if int(v) >= 0]
    rows = []
    for li, lag in enumerate(lags):
        v = sums[li]
        pairs = int(v[0])
        ac, status = autocorr(pairs, *(float(x) for x in v[1:6]))
        half = 1.96 / pairs ** 0.5 if pairs > 0 else None
        rows.append({"summary_level": "matchup", "strategy": None, "matchup_id": int(group_id), "matchup": " | ".join(str(x) for x in ids),
                     "participant_strategy_ids": ids, "n_players": int(k), "observations": int(count), "lagged_pairs": pairs,
                     "lag": int(lag), "metric": "n_rounds", "autocorr": ac, "estimability_status": status,
                     "zero_centered_descriptive_reference_band_lower": -half if half is not None else None,
                     "zero_centered_descriptive_reference_band_upper": half, "sequence_order": MATCHUP_ORDER, "note": note})
    return rows


def stats_table(rows: list[dict[str, Any]]):
    """Rows in the reference's ``_stats_schema`` (:2079-2098)."""
    import pyarrow as pa

    from .rng_lags import stats_schema

    return pa.Table.from_pylist(rows, schema=stats_schema())
