"""The call sequences of tests/call_sequence_cases.py, without a GPU: the driver, the key table and the comparers run every
sequence on the combined CPU engine; the step lists cover what they claim to cover; and two deliberately wrong engines are
caught at the step where they go wrong (the checks of tests/test_call_sequences_gpu.py are thereby shown able to fail)."""
from __future__ import annotations

import numpy as np
import pytest

import call_sequence_cases as cs

ALL = [(g, k, p) for g in "abcdefg" for k in (2, 4) for p in (1, 0)] + [("h", 0, p) for p in (1, 0)]


def _calls(steps) -> list:
    return [(i, s) for i, s in enumerate(steps) if s[0] == "call"]


# ------------------------------------------------------------------------------------------------------------ the CPU engine itself
@pytest.mark.parametrize("group,k,pipeline", ALL, ids=[f"{g}-k{k}-p{p}" for g, k, p in ALL])
def test_every_sequence_on_the_combined_cpu_engine_equals_the_isolated_calls(group, k, pipeline):
    engine = cs.CombinedCpuEngine()  # one engine for the whole group, as on the GPU
    seqs = cs.sequences(group, k, pipeline) + (cs.perm_split_sequences(pipeline) if (group, k) == ("a", 2) else [])
    records_of = {}
    for s in seqs:
        records_of[s.name] = cs.run(engine, s.steps)
        assert all((rec is None) == (step[0] != "call") for rec, step in zip(records_of[s.name], s.steps))
        assert not cs.mismatches(s.name, s.steps, records_of[s.name])
    # the CPU engine prepares nothing: no "wrong" condition is violated; a "consumer" one is (and only through its family)
    for name, index, tag, message in cs.hint_violations(seqs, records_of, pipeline):
        assert tag == "chunks" or (tag in ("consumer", "all_chunks") and pipeline == 1), message


def _arrays(value):
    """The canonical values that are arrays: (shape, bytes)."""
    return None if value is None or isinstance(value, int) else (value[1], value[2])


def test_no_compared_value_is_empty_or_all_zero():
    """Every key of every kind, at both k: an array with elements, not all of them zero; the event list and the pair list hold
    entries; some games end at the safety limit (the overrides' among them)."""
    for k in (2, 4):
        for kind, kd in cs.KINDS.items():
            want = cs.expected(kind, cs.P(k=k, lo=cs.B[0], hi=cs.B[1]))
            assert tuple(want) == kd.keys
            for key, value in want.items():
                if value is None:
                    assert (kind, key, k) in {("seat_counts", "pair_index", 4), ("seat_counts", "pair_sums", 4)}, (kind, key)  # mirrored pairs: k = 2 only
                elif isinstance(value, int):
                    assert value > 0, (kind, key)
                else:
                    shape, data = _arrays(value)
                    assert int(np.prod(shape)) > 0 and any(data), (kind, key, k, shape)
        rare = cs.KINDS["rare_events"].call(cs.CombinedCpuEngine(), dict(cs.P(k=k, lo=cs.B[0], hi=cs.B[1])))["rare_events"]
        assert rare["events"] > 0 and len(rare["event_head"]) == rare["events"] and len(rare["event_seats"]) == rare["events"]
        rows = cs.KINDS["rows"].call(cs.CombinedCpuEngine(), dict(cs.P(k=k, lo=cs.B[0], hi=cs.B[1])))["rows"]
        gps = 64 // k
        assert 0 < int((rows["status"] != 0).sum()) < len(rows)
        for a, b, _ in cs.DEFAULT_OV:  # a game of one or two rounds cannot reach 3 000 points
            assert rows["status"][a * gps + b] != 0 and rows["n_rounds"][a * gps + b] <= 2
    pairs = cs.KINDS["seat_counts"].call(cs.CombinedCpuEngine(), dict(cs.P(k=2, lo=cs.B[0], hi=cs.B[1])))
    assert len(pairs["pair_index"]) > 0 and len(pairs["pair_sums"]) == len(pairs["pair_index"])


def test_the_two_tables_of_64_differ_in_their_packed_form():
    t = cs.tables()
    assert len(t["g64"]) == len(t["g64b"]) == 64 and len(t["g1024"]) == 1024
    assert (t["g64"]["score_threshold"] != t["g64b"]["score_threshold"]).any() and (t["g64b"]["score_threshold"] % 50 == 0).all()
    a = cs.expected("plain", cs.P(table="g64"))
    b = cs.expected("plain", cs.P(table="g64b"))
    assert a != b  # a preparation consumed across the two tables shows in the tally


# ------------------------------------------------------------------------------------------------- coverage of the step lists
def test_every_tournament_kind_consumes_a_right_hint_and_produces_one_at_both_k():
    assert len(cs.TOURNAMENT_KINDS) == 12 and len(cs.NEIGHBOUR_KINDS) == 8
    for pipeline in (1, 0):
        for k in (2, 4):
            for group, hinted_at, other_at in (("a", 1, 0), ("b", 0, 1)):
                seen = set()
                for s in cs.sequences(group, k, pipeline):
                    hint = next(st for st in s.steps if st[0] == "hint")
                    calls = [st for _, st in _calls(s.steps[s.head:])]
                    assert len(calls) == 2 and calls[other_at][1] == "plain"
                    p0, p1 = dict(calls[0][2]), dict(calls[1][2])
                    # a RIGHT hint: the range of the second call, which shares table, k and root with the first
                    assert (hint[1], hint[2]) == (p1["lo"], p1["hi"]) and p0["hi"] <= p1["lo"] and p1["hi"] - p1["lo"] <= p0["hi"] - p0["lo"]
                    assert {key: p0[key] for key in ("table", "k", "root")} == {key: p1[key] for key in ("table", "k", "root")} and p1["k"] == k
                    assert s.checks == [(s.steps.index(calls[1]), "consumer")]
                    seen.add((calls[hinted_at][1], bool(hint[3])))
                assert seen == {(kind, ns) for kind in cs.TOURNAMENT_KINDS for ns in (False, True)}, (group, k)


def test_every_wrong_hint_variant_appears_at_both_k():
    for pipeline in (1, 0):
        for k in (2, 4):
            seqs = cs.sequences("c", k, pipeline)
            names = {s.name.split("/")[1] for s in seqs}
            assert names == set(cs.WRONG_VARIANTS) | set(cs.STILL_VARIANTS) | set(cs.OBSERVED_VARIANTS)
            for s in seqs:
                variant = s.name.split("/")[1]
                hint = next(st for st in s.steps if st[0] == "hint")
                calls = [st for _, st in _calls(s.steps[s.head:])]
                producer, nxt = dict(calls[0][2]), dict(calls[1][2])
                options = {st[1] for st in s.steps[s.steps.index(calls[0]):s.steps.index(calls[1])] if st[0] == "option"}
                hinted = dict(producer, lo=hint[1], hi=hint[2])
                differs = {key for key in hinted if hinted[key] != nxt[key]} | options
                want = {"other_range": {"lo", "hi"}, "same_begin_other_end": {"hi"}, "other_root": {"root"}, "other_k": {"k"}, "other_table": {"table"},
                        "longest_first": {"longest_first"}, "chunk_bytes": {"chunk_bytes"}, "fresh_copy": {"copy"},
                        "other_limits": {"target", "rounds", "ov"}, "hinted_longer": set()}[variant]
                assert differs == want, (s.name, differs)  # exactly one thing
                if variant in cs.WRONG_VARIANTS:
                    assert dict(calls[2][2]) == hinted and (s.steps.index(calls[1]), "wrong") in s.checks  # ... then the hinted call after all
                else:
                    assert s.checks == [(s.steps.index(calls[1]), "observe" if variant in cs.OBSERVED_VARIANTS else "consumer")]
                    if variant == "hinted_longer":
                        assert nxt["hi"] - nxt["lo"] > producer["hi"] - producer["lo"]
                    else:  # the hinted range is no longer than the producing call's: the preparation covers its first chunk
                        assert nxt["hi"] - nxt["lo"] <= producer["hi"] - producer["lo"]


def test_every_neighbour_stands_between_a_hint_and_its_use_alone_and_in_a_pair():
    for k in (2, 4):
        alone, first, second = set(), set(), set()
        for s in cs.sequences("d", k, 1):
            hint = next(st for st in s.steps if st[0] == "hint")
            calls = [st for _, st in _calls(s.steps[s.head:])]
            between = [c[1] for c in calls[1:-1]]
            assert calls[0][1] == "plain" and all(n in cs.NEIGHBOUR_KINDS for n in between) and 1 <= len(between) <= 2
            last = dict(calls[-1][2])
            assert (hint[1], hint[2]) == (last["lo"], last["hi"]) and calls[-1][1] in ("plain", "rows")
            if len(between) == 1:
                alone.add((between[0], calls[-1][1]))
            else:
                first.add(between[0]), second.add(between[1])
        assert alone == {(n, c) for n in cs.NEIGHBOUR_KINDS for c in ("plain", "rows")}
        assert first == second == set(cs.NEIGHBOUR_KINDS)


def test_the_walks_take_every_ordered_pair_of_tournament_kinds():
    """A pair counts when the two calls are neighbours in a walk: only hints and options between them."""
    pairs, hints, kinds = set(), {"right": 0, "wrong": 0, "none": 0}, set()
    for w in cs.walks(1):
        assert 90 <= len(w.steps) <= 130
        calls = [st for _, st in _calls(w.steps)]
        for a, b in zip(calls, calls[1:]):
            if cs.KINDS[a[1]].tournament and cs.KINDS[b[1]].tournament:
                pairs.add((a[1], b[1]))
        kinds |= {c[1] for c in calls}
        for i, st in enumerate(w.steps):
            if st[0] == "call" and cs.KINDS[st[1]].tournament:
                hint = w.steps[i - 1] if w.steps[i - 1][0] == "hint" else None
                nxt = next((c for c in w.steps[i + 1:] if c[0] == "call" and cs.KINDS[c[1]].tournament), None)
                if hint is None or nxt is None:
                    hints["none"] += 1
                else:
                    p, q = dict(st[2]), dict(nxt[2])
                    right = (hint[1], hint[2]) == (q["lo"], q["hi"]) and (p["table"], p["k"], p["root"]) == (q["table"], q["k"], q["root"])
                    hints["right" if right else "wrong"] += 1
    assert pairs == {(a, b) for a in cs.TOURNAMENT_KINDS for b in cs.TOURNAMENT_KINDS}
    assert kinds == set(cs.KINDS)  # every neighbour occurs too
    assert min(hints.values()) >= 20, hints
    tables = {dict(st[2])["table"] for w in cs.walks(1) for _, st in _calls(w.steps)}
    ks = {dict(st[2])["k"] for w in cs.walks(1) for _, st in _calls(w.steps)}
    assert tables == {"g64", "g64b"} and ks == {2, 4}
    assert [w.steps[1:] for w in cs.walks(0)] == [w.steps[1:] for w in cs.walks(1)]  # the same walks with the pipeline off


def test_every_option_a_sequence_sets_is_restored_by_the_gpu_tests():
    names = {st[1] for g, k, p in ALL for s in cs.sequences(g, k or 2, p) for st in s.steps if st[0] == "option"}
    names |= {st[1] for s in cs.perm_split_sequences(1) for st in s.steps if st[0] == "option"}
    assert names == {name for name, _ in cs.RESTORE}


def test_every_scripted_sequence_begins_with_a_table_change():
    """... so that no preparation of an earlier sequence is there to be consumed (the walks begin with whatever there is)."""
    for g, k, p in ALL:
        for s in cs.sequences(g, k or 2, p) + cs.perm_split_sequences(p):
            assert s.steps[0] == ("option", "pipeline", p)
            if g != "h":
                flush, first = s.steps[1], next(st for st in s.steps[s.head:] if st[0] == "call")
                assert s.head == 2 and flush[0] == "call" and dict(flush[2])["table"] == "g64b" and dict(first[2])["table"] in ("g64", "g1024")


# ------------------------------------------------------------------------------------------------------------ detector checks
def _flagged(engine, seq, pipeline=1):
    records = cs.run(engine, seq.steps)
    wrong_results = {i for i, _ in cs.mismatches(seq.name, seq.steps, records)}
    conditions = {(i, tag) for _, i, tag, _ in cs.hint_violations([seq], {seq.name: records}, pipeline) if tag != "chunks"}
    return wrong_results, conditions


@pytest.mark.parametrize("k", [2, 4])
def test_a_stale_preparation_is_caught_in_every_wrong_hint_variant(k):
    """``StaleEngine`` answers the call behind a hinted call's producer from the preparation whenever the begin shuffle matches.
    The wrong call of every variant is flagged: by its RESULT where the variant changes one (end, root, k, table; any range once the
    engine does not even look at the begin), and by the ``prefetched_chunks`` condition in all of them — the only witness where the
    stale answer happens to be the right one (``longest_first``, ``chunk_bytes``: the CPU statement has no schedule and no chunks)."""
    by_result = {"same_begin_other_end", "other_root", "other_k", "other_table"}
    for s in cs.sequences("c", k, 1):
        variant = s.name.split("/")[1]
        step = next(i for i, tag in s.checks if tag == "wrong") if variant in cs.WRONG_VARIANTS else s.checks[-1][0]
        results, conditions = _flagged(cs.StaleEngine("begin"), s)
        if variant == "other_range":  # the begin differs: this engine is right here ...
            assert not results and not conditions
            results, conditions = _flagged(cs.StaleEngine("any"), s)  # ... and the one that does not look at the begin is not
            assert step in results and (step, "wrong") in conditions
        elif variant in cs.WRONG_VARIANTS:
            assert (step, "wrong") in conditions, s.name
            assert (step in results) == (variant in by_result), (s.name, results)
        elif variant == "other_limits":  # still consumed: the limits of the preparing call must not stick to the preparation
            assert results == {step} and not conditions, s.name
        else:  # a fresh copy of the table, a hinted range longer than the producer's: consumed, and right
            assert not results and not conditions, s.name
        assert not cs.mismatches(s.name, s.steps, cs.run(cs.CombinedCpuEngine(), s.steps))


def test_a_result_that_a_neighbour_call_spoils_is_caught_in_every_neighbour_sequence():
    for k in (2, 4):
        for s in cs.sequences("d", k, 1):
            results, _ = _flagged(cs.ResidueEngine(), s)
            assert results == {len(s.steps) - 1}, (s.name, results)  # the hinted call behind the neighbours, and no other step
    walk = cs.walks(1)[0]
    results, _ = _flagged(cs.ResidueEngine(), walk)
    after = {next(j for j in range(i + 1, len(walk.steps)) if walk.steps[j][0] == "call" and cs.KINDS[walk.steps[j][1]].tournament)
             for i, st in _calls(walk.steps) if not cs.KINDS[st[1]].tournament}
    assert results == after and results


def test_the_consumed_table_reads_the_consuming_call():
    s = cs.sequences("a", 2, 1)[0]
    records = cs.run(cs.StaleEngine("begin"), s.steps)
    assert cs.consumed_table([s], {s.name: records}) == {s.family: {False: 1}}
