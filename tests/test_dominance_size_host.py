"""The sparse oracle (tests/dominance_sparse_oracle.py) and the size cases (tests/dominance_size_cases.py) on the CPU: the oracle equals
the host statement ``farkle_ii_amd.dominance.graph`` byte for byte on every designed graph of ``dominance_cases.CASES`` — the chain the
reference-recorded golden file holds — and on the size cases the host statement can still run; the closed forms of the ring and the
total order; and the shapes each size case is there for, so that none misses its target silently.  tests/test_dominance_size_gpu.py
holds the device to the same expected values."""
from __future__ import annotations

import numpy as np
import pytest

import dominance_cases as cases
import dominance_size_cases as size_cases
import dominance_sparse_oracle as oracle
from farkle_ii_amd import dominance as dom

RING, HALF = size_cases.RING, size_cases.RING // 2


def _equal(got: dict, want: dict) -> None:
    for key in ("nodes", "extremes", "adjacency"):
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key


def _host(c: dict, rank) -> dict:
    return dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=rank)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_equals_the_host_statement_on_the_golden_cases(name):
    c = cases.case(name)
    edges = size_cases.edges_of_classes(c["n"], c["cls"])
    for rank in (dom.rank_of_ids(c["ids"]), None):
        _equal(oracle.graph(c["n"], edges, c["low"], c["high"], c["rate"], c["delta"], rank), _host(c, rank))


@pytest.mark.parametrize("name", ["thresholds_1024", "thresholds_1025", "dense_1100", "total_order_1100"])
def test_oracle_equals_the_host_statement_on_the_size_cases_it_can_run(name):
    c = size_cases.case(name)
    _equal(size_cases.expected(name), _host(c, dom.rank_of_ids(c["ids"])))


def test_the_edge_list_of_a_size_case_is_its_classes():
    for name in ("thresholds_1025", "dense_1100"):
        c = size_cases.case(name)
        got = sorted(zip(*(a.tolist() for a in c["edges"])))
        assert got == sorted(zip(*(a.tolist() for a in size_cases.edges_of_classes(c["n"], c["cls"]))))
        assert np.array_equal(np.isnan(c["rate"]), c["cls"] == 6) and np.array_equal(np.isnan(c["low"]), c["cls"] == 6)


def test_oracle_rank_is_the_package_rank():
    c = size_cases.case("thresholds_1025")
    _equal(size_cases.expected("thresholds_1025"), oracle.of_case(c, rank=dom.rank_of_ids(c["ids"])))
    assert not np.array_equal(dom.rank_of_ids(c["ids"]), np.arange(c["n"]))


# ---- closed forms ----
def test_closed_form_of_the_ring_on_a_ring_the_oracle_can_search():
    """``ring_structure`` is what the oracle finds, at a size where its search per member is affordable."""
    n = 130
    i = np.arange(n)
    c = size_cases.build(n, i, (i + 1) % n, np.ones(n, dtype=bool), seed=3)
    _equal(oracle.of_case(c, structures=[size_cases.ring_structure(n)] * 2), oracle.of_case(c))
    _equal(oracle.of_case(c), _host(c, dom.rank_of_ids(c["ids"])))


def test_closed_form_of_ring_4160():
    c, e = size_cases.case("ring_4160"), size_cases.expected("ring_4160")
    n = c["n"]
    assert n == 4160 and np.array_equal(c["edges"][1], (c["edges"][0] + 1) % n) and c["edges"][2].all() and (np.bincount(c["cls"], minlength=7)[[2, 3, 4, 6]] == 0).all()
    nodes = e["nodes"]
    for g in range(2):
        assert (nodes["component"][:, g] == 0).all() and (nodes["component_size"][:, g] == n).all() and (nodes["cycle_length"][:, g] == n).all()
        assert (nodes["front"][:, g] == 1).all() and (nodes["wins"][:, g] == 1).all() and (nodes["losses"][:, g] == 1).all()
        assert (e["adjacency"][g].view(np.uint8) != 0).sum() == n and e["extremes"][g, 0]["strongest_winner"] != oracle.NONE
    assert (nodes["rate_count"] == n - 1).all()
    # many edges share the largest distance: rank decides
    assert e["extremes"][0, 0].tobytes() != oracle.of_case(c, rank=None, structures=[size_cases.ring_structure(n)] * 2)["extremes"][0, 0].tobytes()


def test_closed_form_of_total_order_1100():
    n = 1100
    nodes = size_cases.expected("total_order_1100")["nodes"]
    assert np.array_equal(nodes["front"][:, 1], np.arange(n) + 1) and np.array_equal(nodes["wins"][:, 1], n - 1 - np.arange(n))
    assert np.array_equal(nodes["losses"][:, 1], np.arange(n))
    assert (nodes["component_size"] == 1).all() and np.array_equal(nodes["component"][:, 0], np.arange(n)) and (nodes["cycle_length"] == 0).all()
    assert nodes["front"][:, 1].max() > 1024  # more Kahn rounds than the front kernel has threads


# ---- the shapes the cases are there for ----
@pytest.mark.parametrize("n", size_cases.THRESHOLD_SIZES)
def test_shapes_of_thresholds(n):
    name = f"thresholds_{n}"
    c, e = size_cases.case(name), size_cases.expected(name)
    nodes = e["nodes"]
    table_order = oracle.of_case(c, rank=None)
    centres = size_cases.ring_centres(n)
    fitting = [t for t in size_cases.THRESHOLDS if t in centres]
    assert fitting == [t for t in size_cases.THRESHOLDS if t + HALF < n - RING] and 64 in fitting and centres[-1] == n - 1 - HALF
    for centre in centres:
        lo, hi = centre - HALF, centre + HALF
        for g in range(2):  # a component of nine in BOTH graphs, with rows on both sides of its centre
            assert (nodes["component"][lo:hi + 1, g] == lo).all() and (nodes["component_size"][lo:hi + 1, g] == RING).all()
            assert (nodes["component"][:, g] == lo).sum() == RING and lo < centre < hi
            assert len(set(nodes["cycle_length"][lo:hi + 1, g].tolist())) >= 2
            # the strongest and the weakest edge are decided by rank: in table order another edge takes the place
            by_rank, by_row = e["extremes"][g, lo], table_order["extremes"][g, lo]
            assert by_rank["strongest_distance"] == by_row["strongest_distance"] == (c["delta"] + size_cases.CHORD_UNITS / 1024.0) - c["delta"]
            assert (by_rank["strongest_winner"], by_rank["strongest_loser"]) != (by_row["strongest_winner"], by_row["strongest_loser"])
            assert (by_rank["weakest_winner"], by_rank["weakest_loser"]) != (by_row["weakest_winner"], by_row["weakest_loser"])
        # other threads of the front kernel lower the ring's in-degree: edges into it from rows that are not the head's thread
        w, l, _ = c["edges"]
        entering = w[(l >= lo) & (l <= hi) & ((w < lo) | (w > hi))]
        assert (entering < lo).all() and len(set((entering % 1024).tolist()) - {lo % 1024}) >= (3 if lo >= 130 else 1)
    if n > 1024:  # row 1024, thread 0's second node in the front kernel, is in a ring
        assert (nodes["component_size"][1024] == RING).all()
    # the statistical graph holds the whole path: one front per component, n - 8 k with k rings of nine, which is the most ANY graph
    # with these rings has.  So the fronts pass 1 024 (more Kahn rounds than threads) from 4 096 rows on and 4 096 at 8 192 rows; a
    # table of 1 025 rows with two such rings, or of 4 097 with three, cannot.  The practical graph holds part of the path.
    deepest = int(nodes["front"][:, 1].max())
    assert deepest == n - (RING - 1) * len(centres) and 1 < nodes["front"][:, 0].max() < deepest
    assert (deepest > 1024) == (n >= 4096) and (deepest > 4096) == (n == 8192)
    assert (c["cls"] == 6).sum() >= n // 2 and nodes["rate_count"].min() < n - 1
    assert 11 * n <= len(w) <= 15 * n and (np.abs(w - l) < size_cases.SPAN).all()


def test_shapes_of_the_dense_cases():
    nodes = size_cases.expected("dense_band_4160")["nodes"]
    lo, hi = size_cases.BAND
    for g in range(2):
        head = nodes["component"][hi - 1, g]
        members = np.flatnonzero(nodes["component"][:, g] == head)
        assert len(members) >= 150 and members.min() < 4096 < members.max() and members.min() >= lo
        assert nodes["cycle_length"][members, g].min() == 3  # short cycles
    assert nodes["component_size"][:60 + RING, 1].max() == RING and nodes["front"][:, 1].max() > 1024
    nodes = size_cases.expected("dense_1100")["nodes"]
    for g in range(2):
        assert nodes["component_size"][:, g].max() > 1000
