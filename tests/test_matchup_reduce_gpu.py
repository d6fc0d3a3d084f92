"""``fk_matchup_reduce`` on the MI355X against the literal reference, on the synthetic records of `matchup_reduce_cases.py`: real
equal digests (the collision split's k + 1 passes, ties on the priority at the cut, the tie extension's batches and the binding's
replay with a larger ``out_capacity``), every seat count 1 .. 16, group lengths at the wave's strides, counts at every bin edge and in
the clamped bin, degenerate shapes, a small call after large ones on the same context, and the entry's own argument checks.
Everything is integer: every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

import matchup_reduce_cases as mc
from test_matchup_reduce_cpu import check_against_literal

from farkle_ii_amd import rng_matchups as rm

pytestmark = pytest.mark.gpu

IDS = np.arange(65_536, dtype=np.int32)  # the identity: a table index is its strategy ID
MAX_PLAYERS = 31
RESULT_ARRAYS = ("histogram", "digest", "seats", "count", "sums")


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


def _same_groups(got: dict, want: dict, cap) -> None:
    g = rm.MatchupGroups.from_reduce(got, IDS, MAX_PLAYERS, cap)
    w = rm.MatchupGroups.from_reduce(want, IDS, MAX_PLAYERS, cap)
    for key in ("k", "lags", "observations", "candidate_groups", "eligible_groups", "histogram"):
        assert getattr(g, key) == getattr(w, key), key
    for key in ("priority", "group_id", "participants", "count", "sums"):
        assert np.array_equal(getattr(g, key), getattr(w, key)), key


@pytest.mark.parametrize("name", mc.NAMES)
def test_hip_reduce_equals_the_literal_reference(eng, name):
    records, k, lags, caps = mc.case(name)
    for cap in caps:
        got = eng.matchup_reduce(records, k, lags, cap)
        check_against_literal(got, name, cap)
        _same_groups(got, rm.host_reduce(records, k, lags, cap), cap)


def _raw(result: dict) -> tuple:
    return tuple(np.ascontiguousarray(result[key]).tobytes() for key in RESULT_ARRAYS) + tuple(
        result[key] for key in ("k", "lags", "observations", "candidate_groups", "eligible_groups"))


def test_hip_small_call_after_large_ones_on_the_same_context(eng):
    """The reduce's device buffers only grow: a later, smaller call must not see what an earlier call left in them."""
    records, k, lags, caps = mc.case("strides")
    first = [_raw(eng.matchup_reduce(records, k, lags, cap)) for cap in caps]
    for cap in caps:
        check_against_literal(eng.matchup_reduce(records, k, lags, cap), "strides", cap)
    for name in ("one_group", "tie_batches_end", "collisions_16"):
        big, bk, blags, bcaps = mc.case(name)
        check_against_literal(eng.matchup_reduce(big, bk, blags, bcaps[-1]), name, bcaps[-1])
    assert [_raw(eng.matchup_reduce(records, k, lags, cap)) for cap in caps] == first
    try:  # one run of equal sort keys holding every tuple: the collision split alone restores the groups
        eng.set_option("matchup_sort_key_mask", 0)
        masked = [_raw(eng.matchup_reduce(records, k, lags, cap)) for cap in caps]
    finally:
        eng.set_option("matchup_sort_key_mask", -1)
    assert masked == first
    assert [_raw(eng.matchup_reduce(records, k, lags, cap)) for cap in caps] == first


def test_hip_matchup_reduce_argument_checks(eng):
    from farkle_ii_amd.backend import FarkleHipError

    records, k, lags, caps = mc.case("strides")
    n = len(records["digest"])
    for bad_k in (0, 17):
        wide = {"digest": records["digest"], "seats": np.zeros((n, bad_k), dtype=np.uint16), "rounds": records["rounds"]}
        with pytest.raises(FarkleHipError):
            eng.matchup_reduce(wide, bad_k, (1,), None)
    for bad in ((), (0, 1), (2, 2), (3, 1), tuple(range(1, 18)), (65_536,)):
        with pytest.raises(FarkleHipError):
            eng.matchup_reduce(records, k, bad, None)
    check_against_literal(eng.matchup_reduce(records, k, lags, caps[-1]), "strides", caps[-1])  # the context is still usable
