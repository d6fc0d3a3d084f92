"""Call sequences on one HIP context (tests/call_sequence_cases.py): hints and every entry point.

Every call step of every sequence is compared, key by key, with the same call made alone on the combined CPU engine; and
``fk_timing.prefetched_chunks`` of the calls behind a hint says whether the preparation was consumed at all: a right hint is (for one
of the two ``need_state`` values at least), a wrong one never, and nothing is with the pipeline off.  The CPU side of the same
step lists — coverage, and two wrong engines that these checks catch — is tests/test_call_sequences_cpu.py."""
from __future__ import annotations

import time

import pytest

import call_sequence_cases as cs

pytestmark = pytest.mark.gpu

K_PIPELINE = [(k, p) for k in (2, 4) for p in (1, 0)]
IDS = [f"k{k}-p{p}" for k, p in K_PIPELINE]


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _restore(engine) -> None:
    for name, value in cs.RESTORE:
        engine.set_option(name, value)


def _run(engine, seqs) -> dict:
    """``run`` of every sequence on the one engine, in order; every option a sequence sets is back at its default afterwards."""
    records_of = {}
    t0 = time.perf_counter()
    try:
        for s in seqs:
            records_of[s.name] = cs.run(engine, s.steps)
    finally:
        _restore(engine)
    calls = sum(1 for s in seqs for st in s.steps if st[0] == "call")
    print(f"{seqs[0].group}: {len(seqs)} sequences, {calls} calls on the engine in {time.perf_counter() - t0:.2f} s")
    return records_of


def _check(engine, seqs, pipeline) -> dict:
    records_of = _run(engine, seqs)
    wrong = [message for s in seqs for _, message in cs.mismatches(s.name, s.steps, records_of[s.name])]
    assert not wrong, f"{len(wrong)} steps differ from the CPU statement:\n" + "\n".join(wrong[:12])
    broken = [message for *_, message in cs.hint_violations(seqs, records_of, pipeline)]
    assert not broken, "\n".join(broken[:12])
    return records_of


def _print_consumed(seqs, records_of) -> None:
    for family, by_state in sorted(cs.consumed_table(seqs, records_of).items(), key=str):
        print("consumed", *family, {("state" if ns else "no state"): n for ns, n in sorted(by_state.items())})


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_a_right_hint_every_consumer(eng, k, pipeline):
    seqs = cs.sequences("a", k, pipeline)
    _print_consumed(seqs, _check(eng, seqs, pipeline))


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_b_every_producer(eng, k, pipeline):
    seqs = cs.sequences("b", k, pipeline)
    _print_consumed(seqs, _check(eng, seqs, pipeline))


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_c_wrong_hints_and_the_two_that_are_still_right(eng, k, pipeline):
    seqs = cs.sequences("c", k, pipeline)
    _print_consumed(seqs, _check(eng, seqs, pipeline))


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_d_neighbours_between_a_hint_and_its_use(eng, k, pipeline):
    _check(eng, cs.sequences("d", k, pipeline), pipeline)


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_e_multi_chunk_calls_on_both_sides_of_a_hint(eng, k, pipeline):
    _check(eng, cs.sequences("e", k, pipeline), pipeline)


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_f_a_hint_and_nothing_after_it(eng, k, pipeline):
    _check(eng, cs.sequences("f", k, pipeline), pipeline)


@pytest.mark.parametrize("k,pipeline", K_PIPELINE, ids=IDS)
def test_g_async_images_between_rows_and_plain_calls(eng, k, pipeline):
    _check(eng, cs.sequences("g", k, pipeline), pipeline)


@pytest.mark.parametrize("pipeline", [1, 0])
def test_draws_and_chain_free_permutations_under_hints(eng, pipeline):
    _check(eng, cs.perm_split_sequences(pipeline), pipeline)


@pytest.mark.parametrize("pipeline", [1, 0])
def test_h_three_seeded_walks(eng, pipeline):
    _check(eng, list(cs.walks(pipeline)), pipeline)


def test_h_the_walks_return_the_same_bytes_on_a_fresh_context_and_on_a_used_one(eng):
    """``eng`` has run the other groups (or whatever the suite ran before); the fresh context has run nothing."""
    from farkle_ii_amd import engine as eng_mod

    walks = list(cs.walks(1))
    used = _check(eng, walks, 1)
    eng_mod.set_engine(None)
    try:
        fresh_engine = eng_mod.get_engine()
        assert fresh_engine is not eng
        try:
            fresh = _check(fresh_engine, walks, 1)
        finally:
            fresh_engine.close()
    finally:
        eng_mod.set_engine(eng)
    for w in walks:
        for i, (a, b) in enumerate(zip(used[w.name], fresh[w.name])):
            assert (a is None) == (b is None) and (a is None or a["values"] == b["values"]), f"{w.name}: step {i} {w.steps[i]!r}"
