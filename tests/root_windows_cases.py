"""Designed inputs of the two-root stability stage's window estimates (fk_root_window_estimates), shared by
tests/test_root_windows_host.py and tests/test_root_windows_gpu.py.

Counts.  Every count lies in [2^28, 2^30], so a product of two is about 2^58 and the three float sums round at every addition: the
row-by-row order and NumPy's pairwise order then give different bits (``orders_differ`` holds the cases to that), while counts that
real runs produce stay below 2^53 and could not tell the orders apart.  Zero-exposure cells sit in odd rows of matrices with nine
and more rows, so that no window of the cases loses a column's whole support.

Windows.  Per first cell of ``B`` rows: snapshots from row 0 at a quarter, a half and the whole (one pass, several snapshots); the
whole matrix a second time with another ``pairwise_begin`` (two windows that end at one row); a second half and the rows from 1 on
(``row_begin > 0``); ``pairwise_begin`` in {0, S - 1, S} over them.  A second, five-row cell rides along in every call.
"""
from __future__ import annotations

import numpy as np

S_SIZES = (1, 63, 64, 65, 257)
B_SIZES = (1, 2, 3, 9, 129, 8193)
LARGEST_S_AT = {8193: 65}  # the largest input is 8 193 x 65 x 4 matrices


def cell_case(B: int, S: int, seed: int = 0, zeros: bool = True) -> dict:
    """Four int64 ``[B][S]`` matrices that satisfy the reference's conservation laws."""
    rng = np.random.default_rng([B, S, seed, 77])
    exposures = rng.integers(2 ** 29, 2 ** 30, size=(B, S), dtype=np.int64)
    safety = rng.integers(0, 4, size=(B, S), dtype=np.int64)
    wins = rng.integers(2 ** 28, 2 ** 29, size=(B, S), dtype=np.int64)
    if zeros and B >= 9:
        rows, cols = np.arange(B)[:, None], np.arange(S)[None, :]
        empty = (rows % 2 == 1) & ((rows * 7 + cols * 3) % 11 == 0)
        exposures[empty] = safety[empty] = wins[empty] = 0
    return {"wins": wins, "exposures": exposures, "completed": exposures - safety, "safety": safety}


def cells_case(B: int, S: int, seed: int = 0) -> dict:
    """The call's two cells as the engine takes them: lists of matrices per kind."""
    first, second = cell_case(B, S, seed), cell_case(5, S, seed + 1)
    return {name: [first[name], second[name]] for name in ("wins", "exposures", "completed", "safety")}


def windows_case(B: int, S: int) -> np.ndarray:
    """int64 ``[n][4]``: (cell, row_begin, row_end, pairwise_begin)."""
    begins = (0, S - 1, S)
    rows = []
    for end in sorted({max(B // 4, 1), max(B // 2, 1), B}):
        rows.append((0, 0, end))
    rows.append((0, 0, B))  # ends where the last snapshot ends
    if B >= 2:
        rows += [(0, B // 2, B), (0, 1, B), (0, B // 2, B // 2 + 1)]
    rows += [(1, 0, 5), (1, 2, 5), (1, 2, 4)]
    return np.asarray([(cell, start, stop, begins[i % 3]) for i, (cell, start, stop) in enumerate(rows)], dtype=np.int64)


def sizes() -> list:
    return [(B, S) for B in B_SIZES for S in S_SIZES if S <= LARGEST_S_AT.get(B, max(S_SIZES))]


# ---- the case of the issue: S = 7 cut into chunks of 3, 3 and 1 at 12 rows -------------------------------------------------------
CHUNKED_S, CHUNKED_B, CHUNKED_MAX_BYTES = 7, 12, 57 * 12 * 3
CHUNKED_SEED = 4  # (a seed at which the two orders differ in the last column: the host test asserts it)


def chunked_case() -> dict:
    case = cell_case(CHUNKED_B, CHUNKED_S, CHUNKED_SEED, zeros=False)
    return {name: [m] for name, m in case.items()}


def sequential_sums(wins: np.ndarray, exposures: np.ndarray) -> np.ndarray:
    """float64 ``[3]``: the three sums of one column added row by row, in Python floats."""
    total = [0.0, 0.0, 0.0]
    for w, e in zip(wins.astype(np.float64).tolist(), exposures.astype(np.float64).tolist()):
        total = [total[0] + w * w, total[1] + w * e, total[2] + e * e]
    return np.asarray(total, dtype=np.float64)


def pairwise_sums(wins: np.ndarray, exposures: np.ndarray) -> np.ndarray:
    """float64 ``[3]``: the three sums of one column as NumPy sums a vector."""
    w, e = wins.astype(np.float64), exposures.astype(np.float64)
    return np.asarray([np.add.reduce(w * w), np.add.reduce(w * e), np.add.reduce(e * e)], dtype=np.float64)


def orders_differ(wins: np.ndarray, exposures: np.ndarray) -> bool:
    return sequential_sums(wins, exposures).tobytes() != pairwise_sums(wins, exposures).tobytes()


# ---- the reference's frames (tests/golden/root_stability_frames_vectors.json, tools/gen_root_stability_frames_golden.py) ----------
import json  # noqa: E402
import struct  # noqa: E402
from pathlib import Path  # noqa: E402

GOLDEN_PATH = Path(__file__).resolve().parent / "golden" / "root_stability_frames_vectors.json"
GOLDEN = json.loads(GOLDEN_PATH.read_text())
GOLDEN_NAMES = tuple(case["name"] for case in GOLDEN["cases"])


def golden_case(name: str) -> dict:
    return next(case for case in GOLDEN["cases"] if case["name"] == name)


def expand(v) -> list:
    """A fixture column: a list, ``{"const": v, "n": rows}`` or ``{"dict": distinct, "idx": positions}``."""
    if isinstance(v, dict):
        return [v["const"]] * v["n"] if "const" in v else [v["dict"][i] for i in v["idx"]]
    return v


def golden_table(frame: dict):
    """A recorded frame as an Arrow table."""
    import pyarrow as pa

    kinds = {"int64": pa.int64(), "int32": pa.int32(), "double": pa.float64(), "bool": pa.bool_(), "string": pa.string()}
    arrays = []
    for name, kind in frame["schema"]:
        values = expand(frame["columns"][name])
        if kind == "double":
            values = [None if v is None else float.fromhex(v) for v in values]
        arrays.append(pa.array(values, type=kinds[kind]))
    return pa.Table.from_arrays(arrays, names=[name for name, _ in frame["schema"]])


def assert_same_table(got, want, what):
    """Column for column, type for type, null for null, bit for bit."""
    import pyarrow as pa

    assert [(f.name, str(f.type)) for f in got.schema] == [(f.name, str(f.type)) for f in want.schema], what
    assert got.num_rows == want.num_rows, what
    for name in want.schema.names:
        g, w = got.column(name).to_pylist(), want.column(name).to_pylist()
        if want.schema.field(name).type == pa.float64():
            g = [None if v is None else struct.pack("<d", v) for v in g]
            w = [None if v is None else struct.pack("<d", v) for v in w]
        assert g == w, (what, name)


def golden_cells(case: dict):
    from farkle_ii_amd import root_stability as rs
    from farkle_ii_amd.performance_bootstrap import BatchMatrix

    matrices = {}
    for m in case["matrices"]:
        matrices[(m["root"], m["k"])] = BatchMatrix(m["root"], m["k"], np.asarray(m["batch_ids"], dtype=np.int32),
                                                    np.asarray(case["strategies"], dtype=np.int32),
                                                    *[np.asarray(m[kind], dtype=np.int64) for kind in ("wins", "exposures", "completed", "safety")])
    return rs.check_cells(matrices, case["roots"], case["required_k"])


def golden_across(case: dict) -> dict:
    """The fixture's recorded ``np.dot`` columns of every across-k estimate (they hold only on the machine that wrote them)."""
    floats = lambda values: np.asarray([float.fromhex(v) for v in values], dtype=np.float64)  # noqa: E731
    return {label: {scope: (floats(columns["across_k_score"]), floats(columns["across_k_mcse"])) for scope, columns in scopes.items()}
            for label, scopes in case["across_k"].items()}


def golden_settings(case: dict) -> dict:
    return dict(candidate_contribution_size=case["candidate_contribution_size"],
                practical_delta_by_k={int(k): v for k, v in case["practical_delta_by_k"].items()}, delta_across_k=case["delta_across_k"],
                delta_seed_stability=case["delta_seed_stability"], k_aggregation_method=case["k_aggregation_method"],
                declared_k_weights=None if case["k_weights"] is None else {int(k): v for k, v in case["k_weights"].items()},
                controls=case["controls"], matched_count_fractions=case["matched_count_fractions"], stage_batch_bytes=case["stage_batch_bytes"])
