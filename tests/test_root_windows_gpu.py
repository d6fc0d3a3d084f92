"""The two-root stability stage's window estimates on the MI355X: ``fk_root_window_estimates`` through the C-ABI against the NumPy
host statement (farkle_ii_amd/root_stability.py: ``estimate_windows``) on every case of tests/root_windows_cases.py — integers exact,
every float64 by its bits — with narrowed grids (option ``root_windows_grid``), a small call behind a large one on the same context
and every refusal with its message and the outputs untouched."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import root_windows_cases as cases
from test_root_windows_host import assert_same

from farkle_ii_amd import root_stability as rs
from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    engine = get_engine()
    yield engine
    engine.set_option("root_windows_grid", 0)


@pytest.mark.parametrize("B", cases.B_SIZES)
def test_windows_equal_the_host_statement(eng, B):
    """Every column count at this matrix length: snapshots from one first row, two windows that end at one row, windows that begin
    later, ``pairwise_begin`` in {0, S - 1, S}, a second cell in the same call."""
    for b, S in cases.sizes():
        if b != B:
            continue
        mats, windows = cases.cells_case(B, S), cases.windows_case(B, S)
        assert {0, S - 1, S} <= set(windows[:, 3].tolist())
        assert_same(eng.root_window_estimates(**mats, windows=windows), rs.estimate_windows(**mats, windows=windows), (B, S))


def test_the_chunked_large_count_case(eng):
    """S = 7 in chunks of 3, 3 and 1 at 12 rows: the last column in the pairwise order, which differs there from the row-by-row one
    (tests/test_root_windows_host.py asserts that it does)."""
    mats = cases.chunked_case()
    windows = [rs.stage_window(0, start, stop, cases.CHUNKED_S, cases.CHUNKED_MAX_BYTES) for start, stop in ((0, 12), (0, 6), (6, 12), (0, 3), (0, 9))]
    assert windows[0][3] == cases.CHUNKED_S - 1
    got = eng.root_window_estimates(**mats, windows=windows)
    assert_same(got, rs.estimate_windows(**mats, windows=windows), "chunked")
    last = cases.CHUNKED_S - 1
    column = np.asarray([got[name][0, last] for name in rs.WINDOW_SUMS])
    assert column.tobytes() == cases.pairwise_sums(mats["wins"][0][:, last], mats["exposures"][0][:, last]).tobytes()
    assert column.tobytes() != cases.sequential_sums(mats["wins"][0][:, last], mats["exposures"][0][:, last]).tobytes()


def test_narrowed_grids_change_no_bit(eng):
    mats, windows = cases.cells_case(129, 257), cases.windows_case(129, 257)
    want = rs.estimate_windows(**mats, windows=windows)
    for grid in (1, 2, 3, 7):
        eng.set_option("root_windows_grid", grid)
        assert_same(eng.root_window_estimates(**mats, windows=windows), want, grid)
    eng.set_option("root_windows_grid", 0)
    assert_same(eng.root_window_estimates(**mats, windows=windows), want, "full grid")


def test_a_small_call_behind_a_large_one_reuses_the_workspace(eng):
    large, small = cases.cells_case(8193, 65, seed=2), cases.cells_case(2, 1, seed=2)
    for mats, windows in ((large, cases.windows_case(8193, 65)), (small, cases.windows_case(2, 1)), (large, cases.windows_case(8193, 65)[:2])):
        assert_same(eng.root_window_estimates(**mats, windows=windows), rs.estimate_windows(**mats, windows=windows), len(windows))


def refused(call, message):
    with pytest.raises(FarkleHipError, match=message) as caught:
        call()
    assert caught.value.code == FK_ERR_ARG


def test_refusals_come_with_the_host_statement_s(eng):
    mats = cases.cells_case(9, 5)
    good = np.asarray([(0, 0, 9, 5)], dtype=np.int64)
    for window, message in (((2, 0, 1, 0), "window 1: cell 2 of 2"), ((0, 3, 3, 0), "empty or invalid"), ((0, 0, 10, 0), "empty or invalid"),
                            ((0, -1, 4, 0), "empty or invalid"), ((0, 0, 9, 6), "pairwise_begin = 6 outside"), ((0, 0, 9, -1), "pairwise_begin = -1 outside")):
        windows = np.vstack([good, np.asarray([window], dtype=np.int64)])
        refused(lambda: eng.root_window_estimates(**mats, windows=windows), message)
        with pytest.raises(ValueError):  # the host statement refuses the same input
            rs.estimate_windows(**mats, windows=windows)
    for name, value, message in (("wins", -1, "cell 0: a negative count in batch row 4, column 2"),
                                 ("wins", 2 ** 40, "cell 0: wins > completed in batch row 4, column 2"),
                                 ("safety", 5, "cell 0: exposures != completed \\+ safety in batch row 4, column 2")):
        bad = {key: [m.copy() for m in group] for key, group in mats.items()}
        bad[name][0][4, 2] = value
        refused(lambda: eng.root_window_estimates(**bad, windows=good), message)
        with pytest.raises(ValueError):
            rs.estimate_windows(**bad, windows=good)
    huge = {key: [m.copy() for m in group] for key, group in mats.items()}
    huge["exposures"][1][:, 1] = huge["completed"][1][:, 1] = 2 ** 60
    huge["safety"][1][:, 1] = 0
    refused(lambda: eng.root_window_estimates(**huge, windows=good), "cell 1: the exposure total of column 1 passes 2\\^62")
    empty = {key: [m.copy() for m in group] for key, group in mats.items()}
    for group in empty.values():
        group[0][2:4, 3] = 0
    refused(lambda: eng.root_window_estimates(**empty, windows=[(0, 0, 9, 5), (0, 2, 4, 5)]),
            "window 1: root stability scope contains a strategy without positive exposure: column 3")
    refused(lambda: eng.root_window_estimates(**mats, windows=good, S=0), "S must be in")
    refused(lambda: eng.root_window_estimates(**mats, windows=good, batch_counts=[9, 0]), "cell 1: B = 0")
    refused(lambda: eng.root_window_estimates(**mats, windows=np.zeros((0, 4), dtype=np.int64)), "n_windows = 0")
    assert_same(eng.root_window_estimates(**mats, windows=good), rs.estimate_windows(**mats, windows=good), "after the refusals")


def test_refusals_leave_the_outputs_untouched(eng):
    """Below the Python layer, which always hands arrays in: null pointers, and the caller's arrays after a refused call."""
    lib, ctx = eng._lib, eng._ctx
    mats = cases.cells_case(9, 5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pointers = [(C.c_void_p * 2)(*[m.ctypes.data for m in mats[name]]) for name in ("wins", "exposures", "completed", "safety")]
    counts = np.asarray([9, 5], dtype=np.int64)
    windows = np.asarray([(0, 0, 9, 5), (1, 1, 4, 0)], dtype=np.int64)
    totals, sums = np.full((2, 6, 5), -7, dtype=np.int64), np.full((2, 3, 5), -7.5, dtype=np.float64)

    def call(counts=counts, pointers=pointers, windows=windows, n_windows=2, totals=totals, sums=sums, S=5, n_cells=2):
        return lib.fk_root_window_estimates(ctx, n_cells, None if counts is None else p(counts), *pointers, S, n_windows,
                                            None if windows is None else p(windows), None if totals is None else p(totals),
                                            None if sums is None else p(sums))

    one_null = (C.c_void_p * 2)(mats["wins"][0].ctypes.data, None)
    beyond = np.asarray([(0, 0, 9, 5), (1, 1, 6, 0)], dtype=np.int64)
    for result in (call(counts=None), call(windows=None), call(totals=None), call(sums=None), call(pointers=[None] + pointers[1:]),
                   call(pointers=pointers[:3] + [None]), call(pointers=[one_null] + pointers[1:]), call(n_cells=0), call(n_cells=257),
                   call(n_windows=0), call(S=0), call(windows=beyond)):
        assert result == FK_ERR_ARG
        assert (totals == -7).all() and (sums == -7.5).all()
    assert call() == 0
    want = rs.estimate_windows(**mats, windows=windows)
    assert np.array_equal(totals[:, 0, :], want["wins"]) and sums[:, 2, :].tobytes() == want["sum_e2"].tobytes()
