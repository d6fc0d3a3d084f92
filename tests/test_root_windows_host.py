"""The two-root stability stage's window estimates on the CPU: the two summation orders of csrc/fk_root_windows.h (built into
tests/native/root_windows_host_check.hip without a GPU) against NumPy's own ``np.sum(axis=0)`` bit for bit, for chunks of one and of
two columns; the chunk rule of farkle_ii_amd/root_stability.py against a literal loop; the host statement ``estimate_windows``
against the reference's chunked expressions written out, and against ``estimate_scope`` where the rule gives one chunk."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import root_windows_cases as cases
from farkle_ii_amd import root_stability as rs
from farkle_ii_amd.performance_bootstrap import BatchMatrix

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "root_windows_host_check.hip"
ROW_COUNTS = (1, 7, 8, 9, 128, 129, 8192, 8193)
FLOAT_NAMES = rs.WINDOW_SUMS
INT_NAMES = rs.WINDOW_TOTALS


def assert_same(got: dict, want: dict, what):
    for name in INT_NAMES:
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), (what, name)
    for name in FLOAT_NAMES:
        assert got[name].dtype == np.float64 and np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(want[name]).tobytes(), (what, name)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("root_windows") / "root_windows_host_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True, capture_output=True,
                   text=True)
    return exe


def header_walks(checker, columns) -> list:
    """Per column ``(wins, exposures, row_begin, row_ends)``: per snapshot ``(totals int64 [6], sequential float64 [3], pairwise
    float64 [3])`` of the header's two walks."""
    payload = b""
    for wins, exposures, row_begin, ends in columns:
        payload += struct.pack("<QqQ", len(wins), row_begin, len(ends)) + np.asarray(ends, dtype="<i8").tobytes()
        payload += np.asarray(wins, dtype="<i8").tobytes() + np.asarray(exposures, dtype="<i8").tobytes()
    raw = subprocess.run([str(checker)], input=payload, capture_output=True, timeout=120, check=True).stdout
    words = np.frombuffer(raw, dtype="<u8").reshape(-1, 12)
    assert len(words) == sum(len(ends) for *_, ends in columns)
    return [(row[:6].view("<i8"), row[6:9].view("<f8"), row[9:].view("<f8")) for row in words]


def numpy_sums(wins: np.ndarray, exposures: np.ndarray, width: int) -> np.ndarray:
    """float64 ``[3]``: the reference's three sums (:417-433) of one column that lies in a chunk of ``width`` columns."""
    batch_wins = np.repeat(np.asarray(wins[:, None], dtype=np.float64), width, axis=1)
    batch_exposures = np.repeat(np.asarray(exposures[:, None], dtype=np.float64), width, axis=1)
    positive = batch_exposures > 0
    batch_wins, batch_exposures = np.where(positive, batch_wins, 0.0), np.where(positive, batch_exposures, 0.0)
    return np.asarray([np.sum(batch_wins * batch_wins, axis=0)[0], np.sum(batch_wins * batch_exposures, axis=0)[0],
                       np.sum(batch_exposures * batch_exposures, axis=0)[0]], dtype=np.float64)


def test_header_walks_are_numpy_s_bit_for_bit(checker):
    """Chunks of width 2 add row by row, chunks of width 1 take the pairwise order: at every seam of that order, with zero-exposure
    rows, from row 0 and from a later row, with several snapshots from one walk."""
    columns = []
    for R in ROW_COUNTS:
        case = cases.cell_case(R, 2, seed=R)
        ends = sorted({max(R // 3, 1), max(R - 1, 1), R})
        columns.append((case["wins"][:, 0], case["exposures"][:, 0], 0, ends))
        if R >= 9:
            columns.append((case["wins"][:, 1], case["exposures"][:, 1], R // 2, [R // 2 + 1, R]))
    got = iter(header_walks(checker, columns))
    told_apart = 0
    for wins, exposures, row_begin, ends in columns:
        for end in ends:
            totals, sequential, pairwise = next(got)
            w, e = wins[row_begin:end], exposures[row_begin:end]
            assert totals.tolist() == [w.sum(), e.sum(), e.sum(), 0, e.sum() - w.sum(), np.count_nonzero(e > 0)], (len(wins), row_begin, end)
            assert sequential.tobytes() == numpy_sums(w, e, 2).tobytes() == cases.sequential_sums(w, e).tobytes(), (len(wins), row_begin, end)
            assert pairwise.tobytes() == numpy_sums(w, e, 1).tobytes() == cases.pairwise_sums(w, e).tobytes(), (len(wins), row_begin, end)
            told_apart += sequential.tobytes() != pairwise.tobytes()
    assert told_apart >= len(ROW_COUNTS)  # the counts are large enough for the two orders to differ


def test_chunk_rule_is_the_literal_loop():
    """``window_pairwise_begin`` names exactly the columns that the reference's loop (:404-412) hands to np.sum as a chunk of one."""
    seen = set()
    for S in range(1, 12):
        for rows in (1, 2, 3, 5, 12, 13):
            for max_bytes in [0, 1, 56, 57, 58] + [57 * rows * c + d for c in range(1, 12) for d in (-1, 0, 1)] + [16 << 20]:
                chunk = max(1, min(S, max_bytes // max(1, rows * (7 * np.dtype("<i8").itemsize + 1))))
                alone = [start for start in range(0, S, chunk) if min(S, start + chunk) - start == 1]
                begin = rs.window_pairwise_begin(S, rows, max_bytes)
                assert alone == list(range(begin, S)), (S, rows, max_bytes)
                assert rs.window_chunk(S, rows, max_bytes) == chunk
                seen.add("all" if begin == 0 else "none" if begin == S else "last")
    assert seen == {"all", "none", "last"}
    assert rs.window_pairwise_begin(cases.CHUNKED_S, cases.CHUNKED_B, cases.CHUNKED_MAX_BYTES) == cases.CHUNKED_S - 1
    assert rs.stage_window(3, 2, 14, 7, 57 * 12 * 3) == (3, 2, 14, 6)


def chunked_reference(mats: dict, cell: int, start: int, stop: int, max_bytes: int) -> dict:
    """The loop of ``_estimate_matrix_cells`` (:404-433) over one matrix, written out."""
    S = mats["wins"][cell].shape[1]
    out = {name: np.zeros(S, dtype=np.int64) for name in INT_NAMES}
    out.update({name: np.zeros(S, dtype=np.float64) for name in FLOAT_NAMES})
    chunk = max(1, min(S, max_bytes // max(1, (stop - start) * 57)))
    for column_start in range(0, S, chunk):
        column_stop = min(S, column_start + chunk)
        for name in ("wins", "exposures", "completed", "safety"):
            out[name][column_start:column_stop] += np.asarray(mats[name][cell][start:stop, column_start:column_stop]).sum(axis=0, dtype=np.int64)
        batch_wins = np.asarray(mats["wins"][cell][start:stop, column_start:column_stop], dtype=np.float64)
        batch_exposures = np.asarray(mats["exposures"][cell][start:stop, column_start:column_stop], dtype=np.float64)
        positive = batch_exposures > 0
        out["positive_batches"][column_start:column_stop] += positive.sum(axis=0, dtype=np.int64)
        batch_wins = np.where(positive, batch_wins, 0.0)
        batch_exposures = np.where(positive, batch_exposures, 0.0)
        out["sum_w2"][column_start:column_stop] += np.sum(batch_wins * batch_wins, axis=0)
        out["sum_we"][column_start:column_stop] += np.sum(batch_wins * batch_exposures, axis=0)
        out["sum_e2"][column_start:column_stop] += np.sum(batch_exposures * batch_exposures, axis=0)
    out["losses"] = out["exposures"] - out["wins"]
    return out


def test_host_statement_is_the_reference_s_chunked_loop():
    """Any chunk the byte budget gives: one per column, several columns with a lone last one, one chunk for all."""
    kinds = set()
    for B, S in ((12, 7), (13, 9), (9, 1), (16, 4)):
        mats = cases.cells_case(B, S, seed=4)
        for max_bytes in (1, 57 * B * 2, 57 * B * 3, 57 * (B // 2) * 3, 57 * B * (S - 1) if S > 1 else 57, 16 << 20):
            spans = [(0, 0, B), (0, 0, B // 2), (0, B // 2, B), (1, 0, 5), (1, 2, 5)]
            windows = [rs.stage_window(cell, start, stop, S, max_bytes) for cell, start, stop in spans]
            got = rs.estimate_windows(**mats, windows=windows)
            for i, (cell, start, stop) in enumerate(spans):
                want = chunked_reference(mats, cell, start, stop, max_bytes)
                assert_same({name: got[name][i] for name in got}, want, (B, S, max_bytes, cell, start, stop))
                kinds.add(min(windows[i][3], 1) + (windows[i][3] == S))
    assert kinds == {0, 1, 2}


def test_the_chunked_case_tells_the_orders_apart():
    """S = 7 in chunks of 3, 3 and 1 at 12 rows: the last column takes the pairwise order, the others the row-by-row order, and with
    counts of 2^28 to 2^30 the two orders give different bits in the last column — a kernel with one order for all would fail."""
    mats = cases.chunked_case()
    S, B = cases.CHUNKED_S, cases.CHUNKED_B
    window = rs.stage_window(0, 0, B, S, cases.CHUNKED_MAX_BYTES)
    assert window == (0, 0, B, S - 1) and rs.window_chunk(S, B, cases.CHUNKED_MAX_BYTES) == 3
    got = rs.estimate_windows(**mats, windows=[window])
    wins, exposures = mats["wins"][0], mats["exposures"][0]
    assert cases.orders_differ(wins[:, S - 1], exposures[:, S - 1])
    for s in range(S):
        column = np.asarray([got[name][0, s] for name in FLOAT_NAMES])
        order = cases.pairwise_sums if s == S - 1 else cases.sequential_sums
        assert column.tobytes() == order(wins[:, s], exposures[:, s]).tobytes(), s
    assert any(cases.orders_differ(wins[:, s], exposures[:, s]) for s in range(S - 1))
    assert float(got["sum_e2"].max()) > 2.0 ** 53


def test_every_gpu_case_tells_the_orders_apart():
    """From nine rows on (below eight the pairwise order is the row-by-row one) a case has a column in which the orders differ; a
    lone column of nine rows may round alike, so S = 1 is held to it from 129 rows on."""
    for B, S in cases.sizes():
        if B >= 129 or (B >= 9 and S > 1):
            case = cases.cell_case(B, S)
            assert any(cases.orders_differ(case["wins"][:, s], case["exposures"][:, s]) for s in range(min(S, 8))), (B, S)


def matrix(root: int, k: int, case: dict) -> BatchMatrix:
    B, S = case["wins"].shape
    return BatchMatrix(root, k, np.arange(B, dtype=np.int32), np.arange(S, dtype=np.int32) + 100, case["wins"], case["exposures"], case["completed"],
                       case["safety"])


def test_one_chunk_is_estimate_scope_bit_for_bit():
    """With the default byte budget every window of these shapes is one chunk, and ``scope_from_windows`` over the full windows is
    ``estimate_scope``: a root's scope from one window, ``combined_roots`` from both in the order ``0 + a + b``."""
    for B, S in ((1, 1), (2, 5), (9, 1), (13, 9), (129, 65)):
        a, b = cases.cell_case(B, S, seed=1), cases.cell_case(B + 3, S, seed=2)
        mats = {name: [a[name], b[name]] for name in a}
        windows = [rs.stage_window(0, 0, B, S, rs.DEFAULT_STAGE_BATCH_BYTES), rs.stage_window(1, 0, B + 3, S, rs.DEFAULT_STAGE_BATCH_BYTES)]
        assert [w[3] for w in windows] == [S if S > 1 else 0] * 2
        sums = rs.estimate_windows(**mats, windows=windows)
        for scope, members in (((0,), [matrix(11, 3, a)]), ((1,), [matrix(12, 3, b)]), ((0, 1), [matrix(11, 3, a), matrix(12, 3, b)])):
            got, want = rs.scope_from_windows(sums, scope, 3, 0.01), rs.estimate_scope(members, 3, 0.01)
            for name in ("chance_delta", "batch_mcse"):
                assert got[name].tobytes() == want[name].tobytes(), (B, S, scope, name)
            assert got["practical_threshold_position"] == want["practical_threshold_position"]
            assert np.isnan(got["batch_mcse"]).all() == (B == 1 and scope == (0,))  # one batch: no mcse


def test_stage_windows_lists_every_window_once():
    windows, index = rs.stage_windows([5, 13, 8, 6], 9, rs.DEFAULT_STAGE_BATCH_BYTES, (0.25, 0.5, 0.75, 1.0))
    assert windows.dtype == np.int64 and windows.shape == (len(index), 4) and len({tuple(w) for w in windows.tolist()}) == len(windows)
    for cell, count in enumerate([5, 13, 8, 6]):
        for span in [(0, count), (0, 2), (0, 3), (0, 4), (0, 5), (0, count // 2), (count // 2, count)]:  # matched counts 2, 3, 4 and 5
            assert windows[index[(cell, *span)]].tolist() == [cell, *span, 9]
    assert len(windows) == 5 + 7 + 6 + 6  # (0, 5) and (0, 2) twice in cell 0; (0, 4) is cell 2's first half, (0, 3) cell 3's
    with pytest.raises(ValueError, match="at least two batches"):
        rs.stage_windows([5, 1], 9, rs.DEFAULT_STAGE_BATCH_BYTES, (1.0,))


def test_host_refusals():
    mats = cases.cells_case(9, 5)
    good = [(0, 0, 9, 5)]
    for window, message in (((2, 0, 1, 0), "cell 2 of 2"), ((0, 3, 3, 0), "empty or invalid"), ((0, 0, 10, 0), "empty or invalid"),
                            ((0, -1, 4, 0), "empty or invalid"), ((0, 0, 9, 6), "pairwise_begin = 6"), ((0, 0, 9, -1), "pairwise_begin = -1")):
        with pytest.raises(ValueError, match=message):
            rs.estimate_windows(**mats, windows=[good[0], window])
    for name, value, message in (("wins", -1, "negative count"), ("wins", 2 ** 40, "wins > completed"), ("safety", 5, "completed \\+ safety")):
        bad = {key: [m.copy() for m in group] for key, group in mats.items()}
        bad[name][0][4, 2] = value
        with pytest.raises(ValueError, match=message):
            rs.estimate_windows(**bad, windows=good)
    empty = {key: [m.copy() for m in group] for key, group in mats.items()}
    for group in empty.values():
        group[0][2:4, 3] = 0
    with pytest.raises(ValueError, match="window 1: root stability scope contains a strategy without positive exposure"):
        rs.estimate_windows(**empty, windows=[(0, 0, 9, 5), (0, 2, 4, 5)])
    huge = {key: [m.copy() for m in group] for key, group in mats.items()}
    huge["exposures"][0][:, 1] = huge["completed"][0][:, 1] = 2 ** 60
    huge["safety"][0][:, 1] = 0
    with pytest.raises(ValueError, match="passes 2\\^62"):
        rs.estimate_windows(**huge, windows=good)
    assert_same(rs.HostEngine().root_window_estimates(**mats, windows=good), rs.estimate_windows(**mats, windows=good), "after the refusals")


# ---- the frames against the reference's -------------------------------------------------------------------------------------------
def test_the_golden_file_is_data_and_small():
    assert cases.GOLDEN_PATH.stat().st_size < 400_000
    assert cases.GOLDEN_NAMES == ("k23_unequal", "three_batches", "one_strategy", "chunks_3_3_1")
    main = cases.golden_case("k23_unequal")
    assert sorted(len(m["wins"]) for m in main["matrices"]) == [5, 6, 8, 13]  # the matched counts are 2, 3, 4 and 5
    assert cases.expand(main["frames"]["root_matched_count_convergence"]["columns"]["matched_batches_per_root_k"]) == [2, 3, 4, 5]
    assert any(0 in row for m in main["matrices"] for row in m["exposures"])  # zero-exposure cells inside a column
    assert all([row[3] for row in m["wins"]] == [row[4] for row in m["wins"]] for m in main["matrices"])  # two identical columns
    assert main["controls"] and main["k_weights"] and cases.golden_case("three_batches")["candidate_contribution_size"] > 5
    assert len(cases.golden_case("one_strategy")["strategies"]) == 1


def golden_frames(name: str, engine=None):
    case = cases.golden_case(name)
    tables, estimates = rs.diagnostic_tables(engine or rs.HostEngine(), cases.golden_cells(case), across_k=cases.golden_across(case),
                                             **cases.golden_settings(case))
    return case, tables, estimates


@pytest.mark.parametrize("name", cases.GOLDEN_NAMES)
def test_frames_are_the_reference_s(name):
    """The eight frames by the host path: column for column, type for type, null for null, bit for bit."""
    case, tables, _ = golden_frames(name)
    assert sorted(tables) == sorted(case["frames"])
    assert len(tables) == 7 + len(case["required_k"])
    for frame, recorded in case["frames"].items():
        cases.assert_same_table(tables[frame], cases.golden_table(recorded), (name, frame))


def test_nulls_sit_where_the_reference_has_them():
    _, tables, _ = golden_frames("three_batches")
    drift = tables["root_half_drift"].to_pydict()
    across = [i for i, scope in enumerate(drift["estimand_scope"]) if scope == "across_k"]
    assert across and all(drift["k"][i] is None for i in across) and all(drift["k"][i] is not None for i in range(len(drift["k"])) if i not in across)
    first = [i for i, (root, k) in enumerate(zip(drift["root_seed"], drift["k"])) if root == 11 and k == 2.0]  # B = 3: a first half of one batch
    assert first and all(drift["expected_mcse"][i] is None and drift["standardized_drift"][i] is None for i in first)
    assert any(v is not None for v in drift["expected_mcse"])
    assert tables["root_control_movement"].num_rows == 0 and tables["root_control_movement"].num_columns == 0


def test_the_chunked_golden_case_rounds_in_its_last_column():
    """The case with counts of 2^28 to 2^30 and a byte budget of 57 * 12 * 3: S = 7 in chunks of 3, 3 and 1 at 12 rows, and the two
    summation orders differ in the last column of the first cell — so its frames hold the pairwise order to the reference."""
    case = cases.golden_case("chunks_3_3_1")
    assert case["stage_batch_bytes"] == cases.CHUNKED_MAX_BYTES and len(case["strategies"]) == cases.CHUNKED_S
    m = case["matrices"][0]
    exposures = np.asarray(m["exposures"], dtype=np.int64)
    assert exposures.shape == (cases.CHUNKED_B, cases.CHUNKED_S) and 2 ** 28 <= exposures.min() and exposures.max() <= 2 ** 30 + 4
    assert rs.window_pairwise_begin(cases.CHUNKED_S, cases.CHUNKED_B, case["stage_batch_bytes"]) == cases.CHUNKED_S - 1
    last = exposures[:, -1].astype(np.float64)
    total = 0.0
    for v in (last * last).tolist():
        total += v
    assert total != float(np.add.reduce(last * last))


def test_frame_errors_carry_the_reference_s_messages():
    case = cases.golden_case("k23_unequal")
    cells, settings = cases.golden_cells(case), cases.golden_settings(case)
    for change, message in (({"controls": [999]}, "declared control 999 lacks complete two-root support"),
                            ({"delta_across_k": None}, "screening.delta_across_k is required"),
                            ({"practical_delta_by_k": None}, "screening.practical_delta_by_k is required")):
        with pytest.raises(ValueError, match=message):
            rs.diagnostic_tables(rs.HostEngine(), cells, **{**settings, **change})
    one = cases.golden_case("one_strategy")
    short = cases.golden_cells(one)
    key = (one["roots"][0], one["required_k"][0])
    m = short.matrices[key]
    short.matrices[key] = BatchMatrix(m.root_seed, m.k, m.batch_ids[:1], m.strategies, m.wins[:1], m.exposures[:1], m.completed[:1], m.safety[:1])
    with pytest.raises(ValueError, match=f"root {key[0]}, k={key[1]} needs at least two batches for drift"):
        rs.diagnostic_tables(rs.HostEngine(), short, **cases.golden_settings(one))


def test_the_discrepancy_chain_continues_from_the_window_call():
    """The ``ScopeEstimates`` of the window call are ``scope_estimates``' own wherever the chunk rule gives one chunk."""
    for name in ("k23_unequal", "three_batches", "one_strategy"):
        case, _, estimates = golden_frames(name)
        cells, settings = cases.golden_cells(case), cases.golden_settings(case)
        weights = rs.k_weights(settings["k_aggregation_method"], settings["declared_k_weights"], cells.required_k)
        want = rs.scope_estimates(cells, weights, settings["practical_delta_by_k"], settings["delta_across_k"],
                                  across_k=cases.golden_across(case)["full"])
        assert estimates.scopes == want.scopes
        got_frame, want_frame = rs.discrepancies(estimates, cells, 0.03), rs.discrepancies(want, cells, 0.03)
        for column in rs.DISCREPANCY_COLUMNS:
            g, w = ([None if v is None else struct.pack("<d", v) if isinstance(v, float) else v for v in frame[column]] for frame in (got_frame, want_frame))
            assert g == w, (name, column)
