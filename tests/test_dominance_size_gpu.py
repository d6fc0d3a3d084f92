"""``fk_dominance_graph`` and ``fk_rr_dominance`` on the MI355X at the table sizes where the kernels of csrc/fk_dominance.h change shape:
a front-kernel thread that owns several nodes and more Kahn rounds than threads (n > 1 024), a second trip of the per-row lane loops,
live words in the second wave of the cycle workgroup and pivot blocks past 63 (n > 4 096), every compile-time limit full (n = 8 192),
and the work buffers reused by a small table after the largest.  Expected values: the sparse oracle of tests/dominance_sparse_oracle.py
(held to the host statement and the golden chain by tests/test_dominance_size_host.py), the closed form for the 4 160-row ring;
``nodes``, ``extremes`` and ``adjacency`` byte-equal.  Every call is a valid one."""
from __future__ import annotations

import numpy as np
import pytest

import dominance_cases as cases
import dominance_size_cases as size_cases
import round_robin_engine_stub as stub
import rr_inference_cases as ri_cases
from farkle_ii_amd import dominance as dom

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


def _equal(dev: dict, want: dict, keys=("nodes", "extremes", "adjacency")) -> None:
    for key in keys:
        assert dev[key].shape == want[key].shape and dev[key].tobytes() == want[key].tobytes(), key


def _run(eng, c: dict, **more) -> dict:
    return eng.dominance_graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]), **more)


def _host(c: dict) -> dict:
    return dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]))


@pytest.mark.parametrize("name", list(size_cases.SIZE_CASES))
def test_graph_stage_against_the_sparse_oracle(eng, name):
    dev = _run(eng, size_cases.case(name))
    print(f"{name}: device work {eng.timing()['total_ms']:.2f} ms")
    _equal(dev, size_cases.expected(name))


def test_small_tables_after_the_largest_reuse_its_buffers(eng):
    """W shrinks from 128 to 1 in buffers grown for 8 192 rows; then 1 025 rows, and 4 097 without the adjacency."""
    _equal(_run(eng, size_cases.case("thresholds_8192")), size_cases.expected("thresholds_8192"))
    for name in ("cycle3_and_tail", "sparse_65", "component_across_a_word_boundary"):
        c = cases.case(name)
        _equal(_run(eng, c), _host(c))
    c = size_cases.case("thresholds_1025")
    _equal(_run(eng, c), _host(c))
    dev = _run(eng, size_cases.case("thresholds_4097"), want_adjacency=False)
    assert dev["adjacency"] is None
    _equal(dev, size_cases.expected("thresholds_4097"), keys=("nodes", "extremes"))


def test_resident_chain_above_the_front_kernels_thread_count(eng):
    """``fk_rr_dominance`` over 530 k resident pairs against ``fk_dominance_graph`` fed with the rows of ``fk_rr_inference``: as
    ``_chain_against_stage`` of tests/test_dominance_gpu.py ties them.  (200 games a block, the family's default: its short blocks
    hold 90 wins, so it has no form below 93 games; the cost does not depend on the counts.)"""
    n, roots, target, cap = ri_cases.random_family(n=1030)
    n_pairs = n * (n - 1) // 2
    knobs = dict(ri_cases.PARAMS)
    eng.rr_counts_reset()
    for st in roots:
        eng.rr_counts_add(stub.random_valid_table(n, 8), st, target, cap)
    rank = dom.rank_of_ids(8 + np.arange(n))
    chain = eng.rr_dominance(rank=rank, **knobs)
    t = eng.timing()
    assert t["play_ms"] == t["total_ms"] > 0.0
    inferred = eng.rr_inference(rows=(0, n_pairs), **knobs)
    rows = inferred["rows"]
    assert len(rows) == n_pairs
    stage = eng.dominance_graph(n, rows["decision_class"], rows["simultaneous_d_low"], rows["simultaneous_d_high"], rows["balanced_a_win_rate"],
                                knobs["practical_delta"], rank=rank)
    _equal(chain, stage)
    assert np.array_equal(chain["class_counts"], inferred["class_counts"])
    assert np.array_equal(chain["nodes"]["wins"][:, 0], inferred["strategies"][:, 0]) and np.array_equal(chain["nodes"]["losses"][:, 0], inferred["strategies"][:, 1])
    assert np.array_equal(chain["nodes"]["wins"][:, 1], inferred["strategies"][:, [0, 2]].sum(axis=1))
    # edges in both graphs, several fronts, and pairs without a rate
    assert chain["nodes"]["wins"][:, 0].sum() > 0 and chain["nodes"]["front"].max() > 1 and chain["nodes"]["rate_count"].min() < n - 1
