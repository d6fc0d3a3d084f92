"""``fk_rr_root_diagnostics`` on the MI355X against the host statement (``farkle_ii_amd.rr_root_diagnostics.diagnose``): the synthetic
family with the roots added as seeds (12, 11), a seed with the top bit, one root, a family of several sort and scan tiles and a row
slice of it, a resident range that starts inside the table; the resident round robin with the option on against
``rr_counts_add(root_seed=...)`` of the states ``fk_h2h_round_robin`` returns; every refusal with its message and a good call after it."""
from __future__ import annotations

import math

import numpy as np
import pytest

import round_robin_engine_stub as stub
import rr_root_diagnostics_cases as cases
from farkle_ii_amd import rr_root_diagnostics as rd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    e.rr_counts_reset()
    e.set_option("rr_keep_roots", 1)
    yield e
    e.rr_counts_reset()
    e.set_option("rr_keep_roots", 0)
    e.close()


def _load(eng, table, roots, seeds, target, cap, **where):
    eng.rr_counts_reset()
    for st, seed in zip(roots, seeds):
        eng.rr_counts_add(table, st, target, cap, root_seed=seed, **where)


def test_synthetic_family_root_a_is_the_smaller_seed(eng):
    case = cases.synthetic()
    table = stub.random_valid_table(case["n"], 5)
    _load(eng, table, case["roots"], case["seeds"], case["target"], case["cap"])  # added as (12, 11)
    dev = eng.rr_root_diagnostics(rows=(0, 66), **cases.PARAMS)
    assert dev["roots"].tolist() == [11, 12]
    cases.compare(dev, case["host"])
    none = eng.rr_root_diagnostics(**cases.PARAMS)  # rows and agreement are nullable
    assert none["rows"] is None and none["agreement"] is None and np.array_equal(none["summary"], dev["summary"])
    assert none["max_abs_discrepancy"] == dev["max_abs_discrepancy"]
    only_rows = eng.rr_root_diagnostics(rows=(3, 40), want_agreement=False, **cases.PARAMS)
    assert only_rows["agreement"] is None and only_rows["rows"].tobytes() == np.ascontiguousarray(dev["rows"][:, 3:40]).tobytes()
    # the combined inference over the same accumulator is what it is without the kept roots
    with_roots = eng.rr_inference(rows=(0, 66), **cases.PARAMS)
    eng.rr_counts_reset()
    eng.set_option("rr_keep_roots", 0)
    try:
        for st in case["roots"]:
            eng.rr_counts_add(table, st, case["target"], case["cap"])
        plain = eng.rr_inference(rows=(0, 66), **cases.PARAMS)
        eng.rr_counts_reset()
    finally:
        eng.set_option("rr_keep_roots", 1)
    assert with_roots["rows"].tobytes() == plain["rows"].tobytes() and np.array_equal(with_roots["strategies"], plain["strategies"])


def test_a_seed_with_the_top_bit_and_one_root(eng):
    case = cases.synthetic()
    table = stub.random_valid_table(case["n"], 5)
    big = (1 << 63) + 7
    _load(eng, table, case["roots"], (big, 3), case["target"], case["cap"])
    dev = eng.rr_root_diagnostics(rows=(0, 66), **cases.PARAMS)
    host = rd.diagnose(case["n"], case["roots"], (big, 3), [case["target"]] * 2, [case["cap"]] * 2, **cases.PARAMS)
    assert dev["roots"].tolist() == [3, big]  # ascending as unsigned 64-bit
    cases.compare(dev, host)
    _load(eng, table, case["roots"][:1], (5,), case["target"], case["cap"])
    dev = eng.rr_root_diagnostics(rows=(0, 66), **cases.PARAMS)
    host = rd.diagnose(case["n"], case["roots"][:1], (5,), [case["target"]], [case["cap"]], **cases.PARAMS)
    assert dev["rows"].shape == (1, 66) and dev["summary"][1:4].tolist() == [0, 0, 0] and (dev["summary"][8:] == 0).all()
    assert math.isnan(dev["max_abs_discrepancy"]) and (dev["agreement"]["root_b_decision"] == rd.DECISION_NONE).all()
    cases.compare(dev, host)


def test_scale_and_row_slice(eng):
    """n = 300, 44 850 pairs, two roots: several sort and scan tiles, fourteen pairs without a test; then a slice of the rows."""
    case = cases.wide()
    table = stub.random_valid_table(case["n"], 8)
    _load(eng, table, case["roots"], case["seeds"], case["target"], case["cap"])
    dev = eng.rr_root_diagnostics(rows=(0, 44_850), **cases.PARAMS)
    assert dev["summary"][0] == 44_850 and dev["summary"][1] == 44_836
    cases.compare(dev, case["host"])
    part = eng.rr_root_diagnostics(rows=(12_345, 13_001), **cases.PARAMS)
    assert part["rows"].tobytes() == np.ascontiguousarray(dev["rows"][:, 12_345:13_001]).tobytes()
    assert part["agreement"].tobytes() == dev["agreement"][12_345:13_001].tobytes()
    assert np.array_equal(part["summary"], dev["summary"]) and part["max_abs_discrepancy"] == dev["max_abs_discrepancy"]


def test_resident_range_that_starts_inside_the_table(eng):
    case = cases.wide()
    table = stub.random_valid_table(case["n"], 8)
    lo, hi = 1_003, 9_130  # inside rows of the pair triangle on both sides
    part = [st[lo:hi] for st in case["roots"]]
    _load(eng, table, part, case["seeds"], case["target"], case["cap"], pair_begin=lo, pair_end=hi)
    dev = eng.rr_root_diagnostics(rows=(lo, hi), **cases.PARAMS)
    host = rd.diagnose(case["n"], part, case["seeds"], [case["target"]] * 2, [case["cap"]] * 2, pair_begin=lo, intervals="bisection", **cases.PARAMS)
    cases.assert_margins(host, cases.PARAMS["family_alpha"])
    assert dev["rows"]["pair_id"][0, 0] == lo and dev["rows"]["pair_id"][1, -1] == hi - 1
    cases.compare(dev, host)


def test_resident_round_robin_keeps_its_roots(eng):
    """DESIGN 5.10's hard case, roots 11 and 12, played with the option on: the diagnostics are byte-equal to those over
    rr_counts_add(root_seed=...) of the states fk_h2h_round_robin returns, and the combined inference to a run with the option off."""
    table = stub.hard_table()
    call = {k: v for k, v in stub.HARD.items() if k != "root_seed"}
    knobs = dict(family_alpha=0.02, practical_delta=0.03, delta_equivalence=0.25, min_candidate_completion_rate=0.5)
    plain = [eng.h2h_round_robin(table, root_seed=root, **call)[0] for root in (11, 12)]
    eng.rr_counts_reset()
    for root in (12, 11):
        eng.h2h_round_robin_resident(table, root_seed=root, **call)
    resident = eng.rr_root_diagnostics(rows=(0, 66), **knobs)
    combined = eng.rr_inference(rows=(0, 66), **knobs)
    _load(eng, table, plain, (11, 12), call["target"], call["max_attempts"])
    added = eng.rr_root_diagnostics(rows=(0, 66), **knobs)
    for name in ("roots", "rows", "agreement", "summary"):
        assert resident[name].tobytes() == added[name].tobytes(), name
    assert np.float64(resident["max_abs_discrepancy"]).tobytes() == np.float64(added["max_abs_discrepancy"]).tobytes()
    tested = (resident["rows"][0]["flags"] & 1) != 0
    assert 0 < tested.sum() < 66 and not tested[0]  # rows 0 and 1 never bank: their pair completes no game
    host = rd.diagnose(12, plain, (11, 12), [call["target"]] * 2, [call["max_attempts"]] * 2, **knobs)
    cases.assert_margins(host, knobs["family_alpha"])
    cases.compare(resident, host)
    eng.rr_counts_reset()
    eng.set_option("rr_keep_roots", 0)
    try:
        for root in (12, 11):
            eng.h2h_round_robin_resident(table, root_seed=root, **call)
        off = eng.rr_inference(rows=(0, 66), **knobs)
        eng.rr_counts_reset()
    finally:
        eng.set_option("rr_keep_roots", 1)
    assert combined["rows"].tobytes() == off["rows"].tobytes() and np.array_equal(combined["class_counts"], off["class_counts"])
    assert np.array_equal(combined["strategies"], off["strategies"])


def test_refusals_name_their_reason_and_leave_the_context_usable(eng):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    case = cases.synthetic()
    table = stub.random_valid_table(case["n"], 5)
    roots, target, cap, want = case["roots"], case["target"], case["cap"], case["host"]

    def refused(match, call, *args, **kwargs):
        with pytest.raises(FarkleHipError, match=match) as err:
            call(*args, **kwargs)
        assert err.value.code == FK_ERR_ARG, match

    def good():  # the accumulator and the slots are what the two good adds left
        dev = eng.rr_root_diagnostics(rows=(0, 66), **cases.PARAMS)
        cases.compare(dev, want)

    eng.rr_counts_reset()
    refused("no resident counts", eng.rr_root_diagnostics, **cases.PARAMS)
    # option off: the counts are resident, no root is kept
    eng.set_option("rr_keep_roots", 0)
    try:
        eng.rr_counts_add(table, roots[0], target, cap, root_seed=12)
        refused("no kept roots", eng.rr_root_diagnostics, **cases.PARAMS)
        refused("rr_keep_roots cannot change while counts are resident", eng.set_option, "rr_keep_roots", 1)
        assert eng.get_option("rr_keep_roots") == 0
        eng.rr_counts_reset()
    finally:
        eng.set_option("rr_keep_roots", 1)
    refused("rr_keep_roots is 0 or 1", eng.set_option, "rr_keep_roots", 2)
    assert eng.get_option("rr_keep_roots") == 1
    # an untracked add
    eng.rr_counts_add(table, roots[0], target, cap, root_seed=12)
    eng.rr_counts_add(table, roots[1], target, cap)
    refused("the root set is untracked", eng.rr_root_diagnostics, **cases.PARAMS)
    # the good state, and what is refused on top of it
    _load(eng, table, roots, case["seeds"], target, cap)
    good()
    refused("rr_keep_roots cannot change while counts are resident", eng.set_option, "rr_keep_roots", 0)
    good()
    refused("root_seed 11 is kept already", eng.rr_counts_add, table, roots[0], target, cap, root_seed=11)
    good()
    refused("2 roots are kept already", eng.rr_counts_add, table, roots[0], target, cap, root_seed=13)
    good()
    call = {k: v for k, v in stub.HARD.items() if k != "root_seed"}
    refused("table, range or family differs", eng.h2h_round_robin_resident, stub.hard_table(), root_seed=14, **call)
    good()
    for bad, match in ((dict(rows=(0, 67)), "row range"), (dict(rows=(70, 80)), "row range"), (dict(family_alpha=0.0), "family_alpha must be in"),
                       (dict(practical_delta=0.0), "practical_delta must be positive"), (dict(delta_equivalence=1.0), "delta_equivalence must be in"),
                       (dict(min_candidate_completion_rate=1.01), "min_candidate_completion_rate must be in"),
                       (dict(family_pair_count=65), "is smaller than the 66 pairs"), (dict(family_pair_count=67), "fixed with the resident counts")):
        refused(match, eng.rr_root_diagnostics, **{**cases.PARAMS, **bad})
    good()
    # a duplicate seed on the first slot's own table, through the resident entry: refused before it plays
    eng.rr_counts_reset()
    hard = stub.hard_table()
    eng.rr_counts_add(hard, np.zeros((66, 2, 5), dtype=np.uint32), call["target"], call["max_attempts"], root_seed=11)
    refused("root_seed 11 is kept already", eng.h2h_round_robin_resident, hard, root_seed=11, **call)
    one = eng.rr_root_diagnostics(**cases.PARAMS)
    assert one["roots"].tolist() == [11] and one["summary"][7] == 0  # still the one root, of blocks that completed nothing
