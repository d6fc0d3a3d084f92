"""The performance stage's point estimates on the CPU: ``np_add_reduce`` of csrc/fk_performance.h (built into
tests/native/performance_host_check.hip without a GPU) against NumPy's own ``np.sum`` / ``np.mean`` / ``np.std`` bit for bit at every
column length of ``performance_cases.B_SIZES``; the host statement and the frames of farkle_ii_amd/performance.py against the
reference's own results (tests/golden/performance_vectors.json, recorded by tools/gen_performance_golden.py), every float by its bits,
every column by name, order and type."""
from __future__ import annotations

import json
import math
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pyarrow as pa
import pytest

import performance_cases as cases
from farkle_ii_amd import performance as pf
from farkle_ii_amd.performance_bootstrap import BatchMatrix, bootstrap_schema

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "performance_host_check.hip"
GOLDEN_PATH = ROOT / "tests" / "golden" / "performance_vectors.json"
GOLDEN = json.loads(GOLDEN_PATH.read_text())


def bits(values) -> list:
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("performance") / "performance_host_check"
    # host side only (the checker launches no kernel), as tests/test_power_plan_host.py builds its checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True, capture_output=True,
                   text=True)
    return exe


def header_sums(checker, vectors) -> np.ndarray:
    """float64 ``[len(vectors)][2]``: the header's add.reduce of each vector and of its squared deviations from sum / n."""
    payload = b"".join(struct.pack("<Q", len(v)) + np.asarray(v, dtype="<f8").tobytes() for v in vectors)
    raw = subprocess.run([str(checker)], input=payload, capture_output=True, timeout=120, check=True).stdout
    return np.frombuffer(raw, dtype="<f8").reshape(len(vectors), 2)


def test_the_case_set_tells_summation_orders_apart():
    """A left-to-right sum differs from NumPy's on every column length from 9 up: a kernel that summed in another order would fail."""
    for B in cases.B_SIZES:
        if B >= 9:
            assert cases.naive_sum_differs(cases.by_k_case(B, 65)), B
    rows = [row for _, deltas, _ in cases.across_cases() if deltas.shape[1] >= 8 for row in deltas]
    assert any(cases.naive_sum(row) != float(np.add.reduce(np.array(row))) for row in rows)


def test_header_sums_are_numpy_s_bit_for_bit(checker):
    """np.sum, np.mean and np.std(ddof=1) through their intermediate sums, at every column length of the cases (and beyond NumPy's
    reduction buffer of 8 192 elements), over the compacted rate vectors the reference hands to np.std."""
    vectors = []
    for B in cases.B_SIZES + (8191, 8192, 8193, 20000):
        case = cases.by_k_case(B, 3, "one" if B in (130, 1100) else "none")
        for s in range(3):
            positive = case["exposures"][:, s] > 0
            vectors.append(case["wins"][positive, s].astype(np.float64) / case["exposures"][positive, s])
    for _, deltas, variances in cases.across_cases():  # the across-k rows: d = 1, 2, 3, 8, 16
        vectors += [np.array(deltas[0]), np.array(variances[0])]
    got = header_sums(checker, vectors)
    for (total, ssd), v in zip(got, vectors):
        n = len(v)
        assert bits(total) == bits(np.sum(v)) == bits(np.add.reduce(v)), n
        assert bits(total / n) == bits(np.mean(v)), n
        x = v - np.add.reduce(v) / n
        assert bits(ssd) == bits(np.add.reduce(x * x)), n
        if n >= 2 and not np.isnan(v).any():
            assert bits(np.sqrt(ssd / (n - 1))) == bits(np.std(v, ddof=1)), n


def test_host_by_k_is_numpy_s_std_on_every_case():
    for B in cases.B_SIZES:
        for zero in cases.ZERO_PATTERNS:
            case = cases.by_k_case(B, 5, zero)
            got = pf.host_by_k(2, **case)
            for s in range(5):
                positive = case["exposures"][:, s] > 0
                rates = case["wins"][positive, s].astype(np.float64) / case["exposures"][positive, s]
                assert got["positive_batches"][s] == len(rates)
                if len(rates) >= 2:
                    assert bits(np.sqrt(got["ssd"][s] / (len(rates) - 1))) == bits(np.std(rates, ddof=1)), (B, zero, s)
            assert np.array_equal(got["losses"], case["exposures"].sum(axis=0) - case["wins"].sum(axis=0))


def test_host_refusals():
    case = cases.by_k_case(9, 5)
    with pytest.raises(ValueError, match="no positive exposure support: column 64"):
        pf.host_by_k(3, **cases.zero_column_case())
    for name, value, message in (("wins", -1, "negative count"), ("wins", 2 * 10 ** 12, "wins > completed"), ("safety", 5, "completed \\+ safety")):
        bad = {key: m.copy() for key, m in case.items()}
        bad[name][4, 2] = value
        with pytest.raises(ValueError, match=message):
            pf.host_by_k(3, **bad)
    deltas, variances = cases.pareto_case("chain", 5, 3), cases.variances_case(5, 3)
    with pytest.raises(ValueError, match="1 to 16 required player counts"):
        pf.host_across_k(np.zeros((2, 17)), np.zeros((2, 17)))
    for bad in (np.inf, np.nan):
        broken = deltas.copy()
        broken[3, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            pf.host_across_k(broken, variances)
    broken = variances.copy()
    broken[0, 0] = -1e-9
    with pytest.raises(ValueError, match="negative or infinite"):
        pf.host_across_k(deltas, broken)


def test_pareto_membership_is_the_reference_s_frontier():
    assert sorted(GOLDEN["pareto"]) == sorted(f"{kind}-n{n}-d{d}" for kind, n, d in cases.GOLDEN_PARETO)
    for kind, n, d in cases.GOLDEN_PARETO:
        got = pf.host_across_k(cases.pareto_case(kind, n, d), cases.variances_case(n, d))["pareto_member"]
        assert "".join("1" if m else "0" for m in got.tolist()) == GOLDEN["pareto"][f"{kind}-n{n}-d{d}"], (kind, n, d)


def test_designed_pareto_sets_have_the_designed_members():
    for d in cases.D_SIZES:
        for n in cases.N_SIZES:
            member = lambda kind: pf.pareto_members(cases.pareto_case(kind, n, d))  # noqa: E731
            assert member("chain").tolist() == [False] * (n - 1) + [True]
            assert member("antichain").all()
            duplicates = member("duplicates")
            assert np.array_equal(duplicates[0:(n // 2) * 2:2], duplicates[1::2])  # a point and its copy share their fate
            if d >= 2 and n >= 2:
                assert not member("late_dominator")[n // 3]  # (its dominator may have one of its own among the random rows)
                last = member("last_tile_dominator")
                assert not last[0] and last[1:].all()
            chains = member("equal_but_one")
            assert chains.sum() == min(n, d) and chains[max(n - d, 0):].all()


def test_maximin_leader_follows_the_reference_s_tolerance():
    for kind in cases.MAXIMIN_KINDS:
        deltas, leader = cases.maximin_case(kind)
        res = pf.host_across_k(deltas, cases.variances_case(*deltas.shape))
        assert res["leader_row"] == leader, kind
        minima = deltas.min(axis=1)
        tied = np.flatnonzero(np.isclose(minima, minima.max(), rtol=0.0, atol=1e-15))
        assert leader == tied.min() and len(tied) == (1 if kind == "outside" else 2)


def decode(recorded: dict) -> pa.Table:
    kinds = {"int64": pa.int64(), "int32": pa.int32(), "double": pa.float64(), "bool": pa.bool_(), "string": pa.string()}
    arrays = []
    for name, kind in recorded["schema"]:
        values = recorded["columns"][name]
        if kind == "double":
            values = [None if v is None else float.fromhex(v) for v in values]
        arrays.append(pa.array(values, type=kinds[kind]))
    return pa.Table.from_arrays(arrays, names=[name for name, _ in recorded["schema"]])


def assert_same_table(got: pa.Table, want: pa.Table, what: str):
    assert [(f.name, str(f.type)) for f in got.schema] == [(f.name, str(f.type)) for f in want.schema], what
    for name in want.schema.names:
        g, w = got.column(name).to_pylist(), want.column(name).to_pylist()
        if want.schema.field(name).type == pa.float64():
            g = [None if v is None else struct.pack("<d", v) for v in g]
            w = [None if v is None else struct.pack("<d", v) for v in w]
        assert g == w, (what, name)


def golden_frames(complete_only: bool, engine=None):
    engine = engine or pf.HostEngine()
    settings = cases.GOLDEN_SCREENING
    tables, estimates = {}, {}
    for k, (batch_ids, strategies, m) in sorted(cases.golden_matrices(complete_only).items()):
        matrix = BatchMatrix(cases.GOLDEN_ROOT, k, np.asarray(batch_ids, np.int32), np.asarray(strategies, np.int32), m["wins"], m["exposures"],
                             m["completed"], m["safety"])
        tables[k], estimates[k] = pf.by_k_frame(engine, matrix, settings["resolution_delta"], settings["practical_delta_by_k"][k])
    across, strategies, _ = pf.across_k_frame(engine, estimates, sorted(estimates), settings["delta_across_k"])
    return tables, across, strategies


@pytest.mark.parametrize("complete_only", [False, True], ids=["with_incomplete", "complete"])
def test_frames_are_the_reference_s(complete_only):
    """Column names, order, Arrow types, nulls and the bits of every float: ``_estimate_one_k_matrix`` and ``_across_k_estimates``."""
    recorded = GOLDEN["complete" if complete_only else "with_incomplete"]
    tables, across, strategies = golden_frames(complete_only)
    assert sorted(recorded["by_k"]) == sorted(str(k) for k in tables)
    for k, table in tables.items():
        assert_same_table(table, decode(recorded["by_k"][str(k)]), f"by_k {k}p")
    assert_same_table(across, decode(recorded["across_k"]), "across_k")
    assert strategies.tolist() == recorded["complete_strategies"]
    mcse_5p = tables[5].column("batch_mcse").to_pylist()
    assert mcse_5p[2] is None and all(v is not None for i, v in enumerate(mcse_5p) if i != 2)  # one positive batch: no mcse


def test_screening_frame_and_payload_are_the_reference_s():
    settings = cases.GOLDEN_SCREENING
    tables, across, strategies = golden_frames(True)
    bootstrap = pa.table(cases.golden_bootstrap_columns(strategies), schema=bootstrap_schema())
    screening = pf.screening_frame(across, bootstrap, tables, sorted(tables), settings["candidate_contribution_size"], settings["delta_across_k"],
                                   settings["practical_delta_by_k"], settings["controls"], settings["mandatory_diagnostics"])
    assert_same_table(screening, decode(GOLDEN["complete"]["screening"]), "screening")
    payload = pf.screening_payload(screening, sorted(tables))
    assert {k: v for k, v in payload.items() if k != "interpretation"} == GOLDEN["complete"]["payload"]
    assert "not tests of equality" in payload["interpretation"]
    ranks = pf.win_rate_ranks(screening)
    assert sorted(ranks.values()) == list(range(1, len(strategies) + 1))
    _, incomplete, _ = golden_frames(False)
    with pytest.raises(ValueError, match=r"incomplete strategies: \[500\]"):
        pf.screening_frame(incomplete, bootstrap, tables, sorted(tables), 4, 0.05, settings["practical_delta_by_k"], [], [])


def test_squared_mcse_is_python_s_power():
    values = np.array([0.1, 3.3e-7, np.nan, 0.0, 1.2345678901234567e-3])
    got = pf.squared_mcse(values.reshape(5, 1))
    assert got.shape == (5, 1) and math.isnan(got[2, 0])
    assert [bits(v) for v in got[[0, 1, 3, 4], 0]] == [bits(float(v) ** 2) for v in values[[0, 1, 3, 4]]]


def test_the_golden_file_is_data_and_small():
    assert GOLDEN_PATH.stat().st_size < 100_000
    assert set(GOLDEN) == {"numpy", "with_incomplete", "complete", "pareto"}
