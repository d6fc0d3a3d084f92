"""The matchup reduce's host statement against a literal restatement of the rule, on synthetic records that reach the edges of
``fk_matchup_reduce`` (`matchup_reduce_cases.py`), and the proof — from the literal reference alone — that every case reaches the
regime it is named for: tied priorities at the cut, the tie extension's batch sizes, zero-pair lags, the clamped bin, both sides of
every bin edge, every seat count."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import matchup_reduce_cases as mc  # noqa: E402

from farkle_ii_amd import rng_matchups as rm  # noqa: E402


def check_against_literal(result: dict, name: str, cap) -> None:
    """A reduce result (device or host) == the literal reference: counts, the whole histogram, the kept groups keyed by tuple, and
    the output in non-decreasing priority."""
    summary, kept = mc.literal(name, cap)
    for key in ("observations", "candidate_groups", "eligible_groups"):
        assert result[key] == summary[key], (name, cap, key)
    assert len(result["count"]) == len(result["digest"]) == len(result["seats"]) == len(result["sums"]) == summary["selected_groups"], (name, cap)
    assert np.array_equal(np.asarray(result["histogram"]), mc.histogram_array(summary)), (name, cap)
    assert mc.kept_groups(result) == kept, (name, cap)
    prio = rm.priority(np.asarray(result["digest"], dtype=np.uint64), result["k"])
    assert np.all(prio[1:] >= prio[:-1]), (name, cap)


@pytest.mark.parametrize("name", mc.NAMES)
def test_host_statement_equals_the_literal_reference(name):
    records, k, lags, caps = mc.case(name)
    for cap in caps:
        check_against_literal(rm.host_reduce(records, k, lags, cap), name, cap)


def _tuples_by_digest(name: str) -> dict:
    records, k, _, _ = mc.case(name)
    out: dict[int, set] = {}
    for d, t in zip(records["digest"].tolist(), records["seats"].reshape(-1, k).tolist()):
        out.setdefault(d, set()).add(tuple(t))
    return out


def test_strides_case_reaches_the_wave_strides_and_zero_pair_lags():
    records, k, lags, caps = mc.case("strides")
    summary, kept = mc.literal("strides", None)
    counts = sorted(c for _, c, _ in kept.values())
    assert counts == [c for c in mc.STRIDE_LENGTHS if c >= 3] and summary["counts"] == list(mc.STRIDE_LENGTHS)
    edges = {63, 64, 65, 128, 129}
    assert edges <= set(counts) and edges <= {c - lag for c in counts for lag in lags}
    # an eligible group shorter than (or as long as) a larger lag has no pair there, and one record more has exactly one
    pairs = {(c, lag): s[li][0] for _, c, s in kept.values() for li, lag in enumerate(lags)}
    assert all(p == max(c - lag, 0) for (c, lag), p in pairs.items())
    assert pairs[(3, 63)] == 0 and pairs[(64, 64)] == 0 and pairs[(65, 64)] == 1 and pairs[(128, 128)] == 0 and pairs[(129, 128)] == 1
    assert pairs[(193, 200)] == 0 and pairs[(264, 200)] == 64 and pairs[(265, 200)] == 65
    assert set(records["rounds"].tolist()) == {0, 1, 17, mc.ROUNDS_MAX}
    assert mc.literal("strides", 4)[0]["selected_groups"] == 4 and caps == (None, 4)


def test_every_seat_count_appears_with_first_and_last_column_pairs():
    assert sorted(mc.case(f"every_k_{k}")[1] for k in range(1, 17)) == list(range(1, 17))
    for k in range(1, 17):
        records, _, lags, _ = mc.case(f"every_k_{k}")
        assert records["seats"].shape[1] == k and lags == (1, 3)
        assert records["seats"].min() == 0 and records["seats"].max() == mc.SEAT_MAX
        shared = [sorted(ts) for ts in _tuples_by_digest(f"every_k_{k}").values() if len(ts) > 1]
        differ = [[j for j in range(k) if a[j] != b[j]] for a, b in shared]
        assert all(len(ts) == 2 for ts in shared)
        n_pairs = 1 if k == 1 else 3
        assert differ.count([0]) == (2 if k == 1 else n_pairs) and differ.count([k - 1]) == (2 if k == 1 else n_pairs)
        summary, _ = mc.literal(f"every_k_{k}", None)
        assert len(mc.tied_runs(summary["priorities"])) >= 1                 # both tuples of a pair eligible: a tie
        assert 0 < summary["eligible_groups"] < summary["candidate_groups"] and summary["eligible_groups"] > 50


@pytest.mark.parametrize("k", [3, 16])
def test_collision_caps_sit_around_the_tied_runs(k):
    name = f"collisions_{k}"
    records, _, lags, caps = mc.case(name)
    summary, _ = mc.literal(name, None)
    minimum, E = summary["minimum"], summary["eligible_groups"]
    by_digest = _tuples_by_digest(name)
    sizes = sorted(len(ts) for ts in by_digest.values() if len(ts) > 1)
    assert sizes == [2, 3, 5, 7, 9, 12, 40] and len(by_digest[0]) == 5 and len(by_digest[mc.U64_MAX]) == 40
    assert any(len(by_digest.get(d + 1, ())) == 12 for d, ts in by_digest.items() if len(ts) == 7)   # adjacent digests d, d + 1
    # eligible and ineligible groups inside every run; tuples of a run differ only in the last or only in the first column
    group_count: dict[tuple, int] = {}
    for t in records["seats"].tolist():
        group_count[tuple(t)] = group_count.get(tuple(t), 0) + 1
    for ts in by_digest.values():
        if len(ts) > 1:
            cs = [group_count[t] for t in ts]
            assert min(cs) < minimum <= max(cs)
            cols = {tuple(j for j in range(k) if a[j] != b[j]) for a in ts for b in ts if a < b}
            assert (k - 1,) in cols and ((0,) in cols or len(ts) < 4)  # (two first-column variants from four tuples on)
    runs = mc.tied_runs(summary["priorities"])
    first, longest = runs[0], max(runs, key=lambda se: se[1] - se[0])
    assert first[0] > 0 and longest[1] - longest[0] >= 8
    tied = {cap: mc.literal(name, cap)[0]["tied_behind_cut"] for cap in caps if cap is not None}
    for s, e in (first, longest):
        assert tied[s] == 0                                   # the cut before the run
        assert tied[s + 1] == e - s - 1                       # on its first member: the rest of the run follows
        assert tied[s + (e - s) // 2 + 1] == e - s - (e - s) // 2 - 1
        assert tied[e - 1] == 1 and tied[e] == 0              # on its last-but-one member, exactly at its end
    assert {E - 1, E, E + 1} <= set(caps) and caps[0] is None
    assert [mc.literal(name, c)[0]["selected_groups"] for c in (None, E, E + 1)] == [E, E, E]
    assert mc.literal(name, E - 1)[0]["selected_groups"] in (E - 1, E)


def test_tie_batches_reach_every_batch_size_of_the_extension():
    for variant in mc.TIE_VARIANTS:
        name = f"tie_batches_{variant}"
        records, k, lags, (cap,) = mc.case(name)
        summary, kept = mc.literal(name, cap)
        E, M = summary["eligible_groups"], summary["selected_groups"]
        assert (k, lags) == (3, (1,)) and 0 < cap < E and summary["candidate_groups"] >= 300
        if variant == "end":   # M reaches E inside the loop, in its second batch; the tied run has the greatest priority of all
            assert M == E and mc.TIE_BATCH < summary["tied_behind_cut"] == mc.TIE_END_GROUPS - mc.TIE_KEPT_OF_RUN < 2 * mc.TIE_BATCH
            assert summary["priorities"][-1] == summary["priorities"][cap - 1]
        else:
            assert summary["tied_behind_cut"] == variant and M == cap + variant < E
            assert summary["priorities"][M] > summary["priorities"][M - 1]
        if variant not in (0, 1):  # (M = cap + ties: with 0 or 1 ties the binding's slack cannot be exceeded)
            assert M > cap + mc.REPLAY_SLACK
        assert sum(1 for _, c, _ in kept.values() if c == 3) >= mc.TIE_KEPT_OF_RUN


def test_bins_cases_reach_every_edge_and_the_clamp():
    summary, kept = mc.literal("bins_edges", None)
    minimum = summary["minimum"]
    assert minimum == 3
    for j in mc.BIN_EDGE_POWERS:
        below, at = minimum + (1 << j) - 2, minimum + (1 << j) - 1
        assert below in summary["counts"] and at in summary["counts"]
        assert mc.literal_bin(at, minimum) == minimum + j and mc.literal_bin(below, minimum) == (minimum + j - 1 if j else 2)
        assert summary["histogram"][minimum + j] >= 1
    assert {1, 2, 3, 4, 5, 9, 10, 17, 18, 33, 34} <= set(summary["counts"]) and summary["histogram"][1] == 1
    assert max(summary["histogram"]) == minimum + 12 < minimum + 64
    summary, kept = mc.literal("bins_clamp", None)
    assert summary["minimum"] == 40002 and summary["eligible_groups"] == 0 and kept == {}
    assert summary["counts"] == [32766, 32767, 32768, 35000]
    assert summary["histogram"] == {32766: 1, 32767: 3}   # 32 767 itself and the two groups of more than 32 767 records


def test_degenerate_cases():
    summary, kept = mc.literal("one_record", None)
    assert summary["observations"] == 1 and summary["candidate_groups"] == 1 and kept == {}
    summary, kept = mc.literal("one_group", None)
    m = mc.ROUNDS_MAX
    assert summary["candidate_groups"] == summary["eligible_groups"] == 1 and summary["observations"] == 200_000
    (_, count, sums), = kept.values()
    assert count == 200_000 and [s[0] for s in sums] == [199_999, 134_466, 134_465]
    assert sums[0] == [199_999, 199_999 * m, 199_999 * m, 199_999 * m * m, 199_999 * m * m, 199_999 * m * m] and sums[0][5] > 1 << 47
    (_, count, sums), = mc.literal("one_group_at_the_largest_lag", None)[1].values()
    assert count == 65_536 and [s[0] for s in sums] == [65_535, 2, 1]
    summary, kept = mc.literal("singletons", None)
    assert summary["candidate_groups"] == summary["observations"] == 70_000 and summary["eligible_groups"] == 0
    assert summary["histogram"] == {1: 70_000}
