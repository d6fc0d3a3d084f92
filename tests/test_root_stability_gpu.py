"""The two-root stability stage's bootstrap families on the MI355X: ``fk_root_stability_bootstrap`` through the C-ABI against the
fixture (the reference's own range writers and reductions) and against the NumPy host statement, every output as bytes — strategy
counts off the tile width, batch counts that differ per cell (1 and > 64 included), ``top_n`` at both ends, the top-N family alone,
``expected`` with NaN / 0 / negative entries, nothing valid at all, all-tied input, counts beyond 32 bits, device blocks of several
sizes, replicate ranges split at arbitrary points, the refusals, and one production-shaped call."""
from __future__ import annotations

import numpy as np
import pytest

import root_stability_cases as rc

from farkle_ii_amd import root_stability as rs
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_hip_fixture_cases_equal_the_reference(eng, case):
    cells = rc.case_cells(case)
    p = rs.project_cells(cells)
    _, _, joint = rc.case_joint(case, cells)
    weights = rc.case_weights(case)
    S = len(cells.strategies)
    for start, stop, member, maxima in rc.case_ranges(case):  # the two range writers' payloads
        got = eng.root_stability_bootstrap(p.roots, p.required_k, p.wins, p.exposures, weights, start, stop, case["top_n"], joint.observed,
                                           joint.expected, joint.observed_across, joint.expected_across, want_membership=True)
        assert got["membership"].shape == (stop - start, 2, S) and got["membership"].tobytes() == member.tobytes()
        assert got["maxima"].shape == (stop - start,) and got["maxima"].tobytes() == maxima.tobytes()
        assert np.array_equal(got["top_counts"], member.sum(axis=0, dtype=np.int64))
    if case["root_discrepancies"] is None:
        return
    for range_size in (None, 50, 7):
        tables = rs.root_stability_tables(eng, cells, range_size=range_size, across_k=rc.case_across(case), **rc.case_kwargs(case))
        for name, table in tables.items():
            assert table.num_rows == case[name]["rows"] > 0 and rc.encode(table) == rc.decode(case[name]), name


def _both(eng, args, **kw):
    return eng.root_stability_bootstrap(*args, **kw), rs.host_root_bootstrap(*args, **kw)


@pytest.mark.parametrize("S,batches_a,batches_b", [(1, {2: 3}, {2: 4}), (63, {2: 5, 3: 1}, {2: 1, 3: 7}),
                                                   (257, {2: 65, 4: 64, 6: 1, 7: 130}, {2: 3, 4: 129, 6: 64, 7: 1}), (1000, {3: 33}, None)],
                         ids=["S1", "S63_B1", "S257_tiles", "S1000"])
def test_hip_equals_the_host_statement(eng, S, batches_a, batches_b):
    ks, wins, exposures = rc.synthetic(S, S, batches_a, batches_b)
    weights = np.random.default_rng(S).dirichlet(np.ones(len(ks))).tolist()
    joint = rc.synthetic_joint(S + 1, len(ks), S)
    for top_n in (1, S, min(7, S)):
        got, want = _both(eng, ((3, 8), ks, wins, exposures, weights, 5, 45, top_n), want_membership=True, **joint)
        assert want["maxima"].shape == (40,) and want["membership"].shape == (40, 2, S)
        rc.assert_same(got, want)
    got, want = _both(eng, ((3, 8), ks, wins, exposures, weights, 0, 19, min(2, S)))  # the top-N family alone
    rc.assert_same(got, want)
    assert got["maxima"] is None and got["membership"] is None
    got, want = _both(eng, ((3, 8), ks, wins, exposures, weights, 2, 21, 0), **joint)  # the joint family as its seam asks: top_n 0
    rc.assert_same(got, want)
    assert not got["top_counts"].any()
    empty = eng.root_stability_bootstrap((3, 8), ks, wins, exposures, weights, 4, 4, 1, want_membership=True, **joint)
    assert empty["maxima"].shape == (0,) and empty["membership"].shape == (0, 2, S) and not empty["top_counts"].any()


def test_hip_nothing_valid_gives_zero_maxima(eng):
    ks, wins, exposures = rc.synthetic(5, 300, {2: 9, 5: 4})
    joint = rc.synthetic_joint(6, 2, 300, odd=False)
    joint["expected"] = np.where(np.arange(600).reshape(2, 300) % 3 == 0, np.nan, np.where(np.arange(600).reshape(2, 300) % 3 == 1, 0.0, -0.5))
    joint["expected_across"] = np.full(300, np.nan)
    got, want = _both(eng, ((1, 2), ks, wins, exposures, [0.5, 0.5], 0, 40, 3), **joint)
    rc.assert_same(got, want)
    assert got["maxima"].tobytes() == np.zeros(40).tobytes()  # +0.0, the reference's default
    joint["expected_across"][17] = 0.25  # one estimand alone
    got, want = _both(eng, ((1, 2), ks, wins, exposures, [0.5, 0.5], 0, 40, 3), **joint)
    rc.assert_same(got, want)
    assert np.all(got["maxima"] > 0.0) and np.all(np.isfinite(got["maxima"])) and len(np.unique(got["maxima"])) > 30
    joint["expected"][1, 5] = 5e-324  # a denormal expected: the quotient overflows to +inf, which is the maximum
    got, want = _both(eng, ((1, 2), ks, wins, exposures, [0.5, 0.5], 0, 40, 3), **joint)
    rc.assert_same(got, want)
    assert np.all(np.isinf(got["maxima"]))


def test_hip_all_tied_input_ranks_by_column(eng):
    S = 130
    ks, wins, exposures = rc.synthetic(9, 1, {2: 6, 3: 70})
    wins = [np.repeat(w, S, axis=1) for w in wins]  # every column the same: every score of a replicate is tied
    exposures = [np.repeat(e, S, axis=1) for e in exposures]
    joint = rc.synthetic_joint(10, 2, S)
    for top_n in (1, 64, S):
        got, want = _both(eng, ((4, 5), ks, wins, exposures, [0.25, 0.75], 0, 24, top_n), want_membership=True, **joint)
        rc.assert_same(got, want)
        assert np.all(got["membership"][:, :, :top_n] == 1) and not got["membership"][:, :, top_n:].any()


def test_hip_counts_beyond_32_bits(eng):
    ks, wins, exposures = rc.synthetic(11, 70, {2: 12, 3: 5}, {2: 7, 3: 66}, low=2 ** 40, high=2 ** 41)
    exposures[1][:, 3] = 2 ** 59  # 5 batches: a total of up to 5 * 2^59 stays below 2^63 and beyond 2^53
    joint = rc.synthetic_joint(12, 2, 70)
    got, want = _both(eng, ((7, 9), ks, wins, exposures, [0.6, 0.4], 0, 32, 5), want_membership=True, **joint)
    rc.assert_same(got, want)


def test_hip_split_ranges_and_device_blocks(eng):
    ks, wins, exposures = rc.synthetic(8, 300, {2: 20, 3: 11, 5: 1}, {2: 1, 3: 80, 5: 9})
    weights = [0.2, 0.5, 0.3]
    joint = rc.synthetic_joint(13, 3, 300)
    args = ((21, 22), ks, wins, exposures, weights)
    want = rs.host_root_bootstrap(*args, 0, 100, 25, want_membership=True, **joint)
    rc.assert_same(eng.root_stability_bootstrap(*args, 0, 100, 25, want_membership=True, **joint), want)
    for cuts in ((0, 1, 17, 18, 64, 100), (0, 50, 100), (0, 7, 100), (0, 99, 100)):
        parts = [eng.root_stability_bootstrap(*args, a, b, 25, want_membership=True, **joint) for a, b in zip(cuts[:-1], cuts[1:])]
        merged = {"top_counts": sum(p["top_counts"] for p in parts), "maxima": np.concatenate([p["maxima"] for p in parts]),
                  "membership": np.concatenate([p["membership"] for p in parts])}
        rc.assert_same(merged, want)
    for block in (8, 24, 40, 64):  # the device's own blocks of the range
        eng.set_option("bootstrap_block", block)
        try:
            rc.assert_same(eng.root_stability_bootstrap(*args, 0, 100, 25, want_membership=True, **joint), want)
        finally:
            eng.set_option("bootstrap_block", 0)


def test_hip_refusals(eng):
    ks, wins, exposures = rc.synthetic(14, 40, {2: 4, 3: 1})
    joint = rc.synthetic_joint(15, 2, 40)
    args = ((1, 2), ks, wins, exposures, [0.5, 0.5])
    assert eng.root_stability_bootstrap(*args, 0, 8, 3, **joint)["maxima"].shape == (8,)

    def refused(match, *a, **kw):
        with pytest.raises(FarkleHipError, match=match) as info:
            eng.root_stability_bootstrap(*a, **kw)
        assert info.value.code == FK_ERR_ARG

    # the `bad` flag: the ONE eligible batch row of cell (root 2, k = 3) has a zero exposure -> every resampled total is zero
    zero = [e.copy() for e in exposures]
    zero[3][0, 7] = 0
    zero_wins = [w.copy() for w in wins]
    zero_wins[3][0, 7] = 0
    refused("zero complete-support exposure", (1, 2), ks, zero_wins, zero, [0.5, 0.5], 0, 8, 3, **joint)
    with pytest.raises(ValueError, match="zero complete-support exposure"):
        rs.host_root_bootstrap((1, 2), ks, zero_wins, zero, [0.5, 0.5], 0, 8, 3, **joint)
    negative = [w.copy() for w in wins]
    negative[2][1, 1] = -1
    refused("negative count", (1, 2), ks, negative, exposures, [0.5, 0.5], 0, 8, 3)
    huge = [e.copy() for e in exposures]
    huge[0][2, 5] = 2 ** 61  # 4 batches: 4 * 2^61 = 2^63
    refused("2\\^63", (1, 2), ks, wins, huge, [0.5, 0.5], 0, 8, 3)
    refused("a < b", (2, 2), *args[1:], 0, 8, 3)
    refused("a < b", (5, 2), *args[1:], 0, 8, 3)
    refused("top_n", *args, 0, 8, 41)
    refused("replicate range", *args, 8, 0, 3)
    refused("weight is not finite", (1, 2), ks, wins, exposures, [0.5, np.nan], 0, 8, 3)
    for name in ("observed", "observed_across"):
        broken = {k: v.copy() for k, v in joint.items()}
        broken[name].reshape(-1)[11] = np.inf
        refused("observed is not finite", *args, 0, 8, 3, **broken)
    rc.assert_same(*_both(eng, (*args, 0, 8, 3), **joint))  # the context is usable after every refusal


def test_hip_production_shape_sampled_against_the_host_statement(eng):
    """2 roots x k in {2,3,4,5,6,8,10,12} x 100 batches, 5 160 strategies, 2 000 replicates in one call; the host statement on 12
    replicates spread over the range (a time cap on the host statement, not a tolerance: the sampled replicates are compared as
    bytes) and the inclusion counts against the call's own membership."""
    S, R = 5160, 2000
    ks = [2, 3, 4, 5, 6, 8, 10, 12]
    _, wins, exposures = rc.synthetic(77, S, {k: 100 for k in ks})
    weights = [1.0 / len(ks)] * len(ks)
    joint = rc.synthetic_joint(78, len(ks), S)
    args = ((7, 19), ks, wins, exposures, weights)
    got = eng.root_stability_bootstrap(*args, 0, R, 75, want_membership=True, **joint)
    assert got["membership"].shape == (R, 2, S) and got["maxima"].shape == (R,) and got["top_counts"].shape == (2, S)
    assert np.array_equal(got["top_counts"], got["membership"].sum(axis=0, dtype=np.int64))
    assert np.all(got["membership"].sum(axis=2) == 75) and np.all(got["maxima"] > 0.0) and np.all(np.isfinite(got["maxima"]))
    assert len(np.unique(got["maxima"])) > R // 2
    sample = [0, 1, 7, 255, 256, 511, 1000, 1023, 1024, 1500, 1998, 1999]
    for r in sample:
        want = rs.host_root_bootstrap(*args, r, r + 1, 75, want_membership=True, **joint)
        assert got["membership"][r].tobytes() == want["membership"][0].tobytes(), r
        assert got["maxima"][r:r + 1].tobytes() == want["maxima"].tobytes(), r
    sums_only = eng.root_stability_bootstrap(*args, 0, R, 75)  # the top-N family alone, no membership: the same counts
    assert np.array_equal(sums_only["top_counts"], got["top_counts"])
