"""``fk_dominance_graph`` and ``fk_rr_dominance`` on the MI355X against the host statement (``farkle_ii_amd.dominance.graph``): every
designed graph of tests/dominance_cases.py with ``nodes``, ``extremes`` and ``adjacency`` bit-equal; a null ``adjacency``; the resident
chain against the graph stage fed with the rows ``fk_rr_inference`` returns, equivalence on and off; every refusal with its message and
a good call after it; a partial resident range refused."""
from __future__ import annotations

import numpy as np
import pytest

import dominance_cases as cases
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


def _equal(dev: dict, host: dict) -> None:
    for key in ("nodes", "extremes", "adjacency"):
        assert dev[key].shape == host[key].shape and dev[key].tobytes() == host[key].tobytes(), key


def _run(eng, c: dict, **more) -> dict:
    return eng.dominance_graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]), **more)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_graph_stage_against_the_host_statement(eng, name):
    c = cases.case(name)
    host = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]))
    _equal(_run(eng, c), host)


def test_table_order_and_null_adjacency(eng):
    c = cases.case("equal_distances")
    host = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"])
    dev = eng.dominance_graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], want_adjacency=False)
    assert dev["adjacency"] is None
    for key in ("nodes", "extremes"):
        assert dev[key].tobytes() == host[key].tobytes(), key
    t = eng.timing()
    assert t["play_ms"] == t["total_ms"] > 0.0 and 0.0 < t["perm_ms"] + t["seed_ms"] <= t["play_ms"]


def _load(eng, table, roots, target, cap, **where):
    eng.rr_counts_reset()
    for st in roots:
        eng.rr_counts_add(table, st, target, cap, **where)


def _chain_against_stage(eng, n: int, knobs: dict) -> dict:
    """``fk_rr_dominance`` over the resident counts against ``fk_dominance_graph`` fed with the rows of ``fk_rr_inference``."""
    rank = dom.rank_of_ids(8 + np.arange(n))
    chain = eng.rr_dominance(rank=rank, **knobs)
    t = eng.timing()
    assert t["play_ms"] == t["total_ms"] > 0.0
    inferred = eng.rr_inference(rows=(0, n * (n - 1) // 2), **knobs)
    rows = inferred["rows"]
    stage = eng.dominance_graph(n, rows["decision_class"], rows["simultaneous_d_low"], rows["simultaneous_d_high"], rows["balanced_a_win_rate"],
                                knobs["practical_delta"], rank=rank)
    _equal(chain, stage)
    assert np.array_equal(chain["class_counts"], inferred["class_counts"])
    assert np.array_equal(chain["nodes"]["wins"][:, 0], inferred["strategies"][:, 0]) and np.array_equal(chain["nodes"]["losses"][:, 0], inferred["strategies"][:, 1])
    assert np.array_equal(chain["nodes"]["wins"][:, 1], inferred["strategies"][:, [0, 2]].sum(axis=1))
    return chain


@pytest.mark.parametrize("equivalence", [None, ri_cases.DELTA_EQUIVALENCE], ids=["equivalence_off", "equivalence_on"])
def test_resident_chain_on_the_synthetic_family(eng, equivalence):
    n, roots, target, cap = ri_cases.synthetic_family()
    _load(eng, stub.random_valid_table(n, 5), roots, target, cap)
    chain = _chain_against_stage(eng, n, dict(delta_equivalence=equivalence, **ri_cases.PARAMS))
    assert chain["nodes"]["wins"].sum() > 0 and chain["nodes"]["rate_count"].min() < n - 1  # edges, and pairs without a rate


@pytest.mark.parametrize("equivalence", [None, ri_cases.DELTA_EQUIVALENCE], ids=["equivalence_off", "equivalence_on"])
def test_resident_chain_on_the_random_family(eng, equivalence):
    n, roots, target, cap = ri_cases.random_family()
    _load(eng, stub.random_valid_table(n, 8), roots, target, cap)
    chain = _chain_against_stage(eng, n, dict(delta_equivalence=equivalence, **ri_cases.PARAMS))
    assert chain["nodes"]["front"].max() > 1


@pytest.mark.parametrize("equivalence", [None, 0.25], ids=["equivalence_off", "equivalence_on"])
def test_resident_chain_on_the_played_hard_table(eng, equivalence):
    table = stub.hard_table()
    call = {k: v for k, v in stub.HARD.items() if k != "root_seed"}
    eng.rr_counts_reset()
    for root in (11, 12):
        eng.h2h_round_robin_resident(table, root_seed=root, **call)
    _chain_against_stage(eng, 12, dict(family_alpha=0.02, practical_delta=0.03, delta_equivalence=equivalence, min_candidate_completion_rate=0.5))


def test_refusals_name_their_reason_and_leave_the_context_usable(eng):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    c = cases.case("cycle3_and_tail")
    host = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]))

    def good():
        _equal(_run(eng, c), host)

    good()
    args = dict(n=c["n"], decision_class=c["cls"], sim_d_low=c["low"], sim_d_high=c["high"], balanced_rate=c["rate"], practical_delta=c["delta"])
    bad_class, bad_low, bad_high = c["cls"].copy(), c["low"].copy(), c["high"].copy()
    bad_class[2] = 7
    bad_low[0] = np.nan  # pair 0 is the practical edge 0 -> 1: it needs its low bound
    flipped = c["cls"].copy()
    flipped[0] = 1       # ... and as an edge 1 -> 0 its high bound
    bad_high[0] = np.inf
    one = dict(n=1, decision_class=np.zeros(0, np.uint8), sim_d_low=np.zeros(0), sim_d_high=np.zeros(0), balanced_rate=np.zeros(0))
    for bad, match in ((one, "at least two strategies"), (dict(n=8193), "at most 8192 strategies"), (dict(decision_class=bad_class), "decision class 7 of pair 2"),
                       (dict(sim_d_low=bad_low), "pair 0 is a practical dominance whose simultaneous bound is not finite"),
                       (dict(decision_class=flipped, sim_d_high=bad_high), "pair 0 is a practical dominance whose simultaneous bound is not finite"),
                       (dict(practical_delta=0.0), "practical_delta must be positive"), (dict(practical_delta=float("nan")), "practical_delta must be positive"),
                       (dict(rank=[0, 1, 1, 3]), "rank is not a permutation"), (dict(rank=[0, 1, 2, 4]), "rank is not a permutation")):
        call = {**args, **bad}  # (a size the entry refuses is refused before an array is read)
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.dominance_graph(**call)
        assert err.value.code == FK_ERR_ARG, match
        good()
    # the resident chain: no counts, a partial range, a bad rank; then a good call
    n, roots, target, cap = ri_cases.synthetic_family()
    table = stub.random_valid_table(n, 5)
    eng.rr_counts_reset()
    with pytest.raises(FarkleHipError, match="no resident counts") as err:
        eng.rr_dominance(**ri_cases.PARAMS)
    assert err.value.code == FK_ERR_ARG
    _load(eng, table, [r[3:60] for r in roots], target, cap, pair_begin=3, pair_end=60)
    with pytest.raises(FarkleHipError, match=r"hold pairs \[3, 60\) of the table's 66: a dominance graph needs the whole family") as err:
        eng.rr_dominance(**ri_cases.PARAMS)
    assert err.value.code == FK_ERR_ARG
    _load(eng, table, roots, target, cap)
    for bad, match in ((dict(rank=np.zeros(n, dtype=np.uint32)), "rank is not a permutation"), (dict(practical_delta=0.0), "practical_delta must be positive"),
                       (dict(family_alpha=1.0), "family_alpha must be in"), (dict(family_pair_count=67), "fixed with the resident counts")):
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.rr_dominance(**{**ri_cases.PARAMS, **bad})
        assert err.value.code == FK_ERR_ARG, match
    _chain_against_stage(eng, n, dict(delta_equivalence=None, **ri_cases.PARAMS))
    good()
