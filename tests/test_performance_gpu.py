"""The performance stage's point estimates on the MI355X: ``fk_performance_by_k`` and ``fk_performance_across_k`` through the C-ABI
against the NumPy host statement (farkle_ii_amd/performance.py) on every case of tests/performance_cases.py — integers exact, every
float64 by its bits — with narrowed grids (option ``performance_grid``), a small call behind a large one on the same context, every
refusal with its message and outputs untouched, and the frames over the golden matrices against the reference's."""
from __future__ import annotations

import numpy as np
import pytest

import performance_cases as cases
import test_performance_host as host_tests

from farkle_ii_amd import performance as pf
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

pytestmark = pytest.mark.gpu

INT_NAMES = ("wins", "exposures", "completed", "safety", "losses", "positive_batches")


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    engine = get_engine()
    yield engine
    engine.set_option("performance_grid", 0)


def assert_by_k(got: dict, want: dict, what):
    for name in INT_NAMES:
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), (what, name)
    for name in ("rate_sum", "ssd"):
        assert got[name].dtype == np.float64 and got[name].tobytes() == want[name].tobytes(), (what, name)


def assert_across(got: dict, want: dict, what):
    for name in ("delta_sum", "variance_sum", "minimum"):
        assert got[name].tobytes() == np.asarray(want[name], dtype=np.float64).tobytes(), (what, name)
    assert np.array_equal(got["worst_index"], want["worst_index"]), what
    assert np.array_equal(got["pareto_member"], want["pareto_member"]), what
    assert got["leader_row"] == want["leader_row"], what


@pytest.mark.parametrize("B", cases.B_SIZES)
def test_by_k_equals_the_host_statement(eng, B):
    """Every column count and every zero-exposure pattern at this column length; the widest table again through two workgroups."""
    for S in cases.S_SIZES:
        for zero in cases.ZERO_PATTERNS:
            case = cases.by_k_case(B, S, zero)
            want = pf.host_by_k(4, **case)
            assert_by_k(eng.performance_by_k(4, **case), want, (B, S, zero))
            if S == 257 and zero == "one":
                for grid in (1, 2, 3):
                    eng.set_option("performance_grid", grid)
                    assert_by_k(eng.performance_by_k(4, **case), want, (B, S, zero, grid))
                eng.set_option("performance_grid", 0)


@pytest.mark.parametrize("kind", cases.PARETO_KINDS + tuple(f"maximin-{kind}" for kind in cases.MAXIMIN_KINDS))
def test_across_k_equals_the_host_statement(eng, kind):
    checked = 0
    for name, deltas, variances in cases.across_cases():
        if name != kind and not name.startswith(kind + "-n"):
            continue
        want = pf.host_across_k(deltas, variances)
        assert_across(eng.performance_across_k(deltas, variances), want, name)
        if deltas.shape[0] > cases.TILE:  # candidate blocks and rows strided over one and two workgroups
            for grid in (1, 2):
                eng.set_option("performance_grid", grid)
                assert_across(eng.performance_across_k(deltas, variances), want, (name, grid))
            eng.set_option("performance_grid", 0)
        checked += 1
    assert checked == (1 if kind.startswith("maximin") else len(cases.D_SIZES) * len(cases.N_SIZES))


def test_maximin_leaders_are_the_designed_ones(eng):
    for kind in cases.MAXIMIN_KINDS:
        deltas, leader = cases.maximin_case(kind)
        assert eng.performance_across_k(deltas, cases.variances_case(*deltas.shape))["leader_row"] == leader, kind


def test_a_small_call_behind_a_large_one_reuses_the_workspace(eng):
    large, small = cases.by_k_case(1100, 257, "all_but_two"), cases.by_k_case(2, 1, "none")
    assert_by_k(eng.performance_by_k(2, **large), pf.host_by_k(2, **large), "large")
    assert_by_k(eng.performance_by_k(2, **small), pf.host_by_k(2, **small), "small")
    rng = np.random.default_rng(5)
    deltas, variances = rng.standard_normal((5160, 8)) * 0.01, rng.random((5160, 8)) * 1e-6  # the production shape
    assert_across(eng.performance_across_k(deltas, variances), pf.host_across_k(deltas, variances), "production shape")
    deltas, variances = cases.pareto_case("duplicates", 1, 1), cases.variances_case(1, 1)
    assert_across(eng.performance_across_k(deltas, variances), pf.host_across_k(deltas, variances), "one row")


def refused(call, message):
    with pytest.raises(FarkleHipError, match=message) as caught:
        call()
    assert caught.value.code == FK_ERR_ARG


def test_by_k_refusals(eng):
    case = cases.by_k_case(9, 5)
    refused(lambda: eng.performance_by_k(3, **cases.zero_column_case()), "3p: strategies have no positive exposure support: column 64")
    for name, value, message in (("wins", -1, "a negative count in batch row 4, column 2"),
                                 ("wins", 2 * 10 ** 12, "wins > completed in batch row 4, column 2"),
                                 ("safety", 5, "exposures != completed \\+ safety in batch row 4, column 2")):
        bad = {key: m.copy() for key, m in case.items()}
        bad[name][4, 2] = value
        refused(lambda: eng.performance_by_k(3, **bad), message)
        with pytest.raises(ValueError):  # the host statement refuses the same input
            pf.host_by_k(3, **bad)
    huge = {key: m.copy() for key, m in case.items()}
    huge["exposures"][:, 1] = huge["completed"][:, 1] = 2 ** 60
    huge["safety"][:, 1] = 0
    refused(lambda: eng.performance_by_k(3, **huge), "the exposure total of column 1 passes 2\\^62")
    refused(lambda: eng.performance_by_k(0, **case), "player count k = 0")
    refused(lambda: eng.performance_by_k(3, **case, B=0), "a batch matrix has 1 to 2\\^31 - 1 batches")
    refused(lambda: eng.performance_by_k(3, **case, S=0), "S must be in")
    assert_by_k(eng.performance_by_k(3, **case), pf.host_by_k(3, **case), "after the refusals")


def test_across_k_refusals(eng):
    deltas, variances = cases.pareto_case("duplicates", 9, 3), cases.variances_case(9, 3)
    refused(lambda: eng.performance_across_k(np.zeros((2, 17)), np.zeros((2, 17))), "d = 17: 1 to 16 required player counts")
    refused(lambda: eng.performance_across_k(deltas, variances, d=0), "d = 0: 1 to 16 required player counts")
    refused(lambda: eng.performance_across_k(deltas, variances, n=0), "n = 0")
    for bad in (np.inf, -np.inf, np.nan):
        broken = deltas.copy()
        broken[7, 2] = bad
        refused(lambda: eng.performance_across_k(broken, variances), "row 7, player count 2: the chance delta is not finite")
    for bad in (-1e-9, np.inf):
        broken = variances.copy()
        broken[0, 1] = bad
        refused(lambda: eng.performance_across_k(deltas, broken), "row 0, player count 1: the variance is negative or infinite")
    assert_across(eng.performance_across_k(deltas, variances), pf.host_across_k(deltas, variances), "after the refusals")


@pytest.mark.parametrize("complete_only", [False, True], ids=["with_incomplete", "complete"])
def test_frames_on_the_device_are_the_reference_s(eng, complete_only):
    recorded = host_tests.GOLDEN["complete" if complete_only else "with_incomplete"]
    tables, across, _ = host_tests.golden_frames(complete_only, engine=eng)
    for k, table in tables.items():
        host_tests.assert_same_table(table, host_tests.decode(recorded["by_k"][str(k)]), f"by_k {k}p")
    host_tests.assert_same_table(across, host_tests.decode(recorded["across_k"]), "across_k")
