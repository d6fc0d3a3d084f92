"""``fk_score_power_scan`` on the MI355X against the host statement (``h2h_power.power_cells_host``): the sizes at which the kernel
changes shape — below, at and above a wave, a workgroup's chunk and several chunks, the last size whose tails fit LDS and the first in
the global workspace, a size of the whole-grid family's order — at the production scenarios, at probabilities whose tails underflow
and at three alphas; a full scan of n = 1 .. 300; the order of the cells, batch sizes, workspace reuse, every refusal; and the plans on
the HIP engine against the reference's recorded results (tests/golden/power_plan_vectors.json)."""
from __future__ import annotations

import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

import power_plan_cases as cases
from farkle_ii_amd import h2h_power as hp
from farkle_ii_amd.backend import FK_ERR_ARG, POWER_CELL_DTYPE, POWER_LDS_MAX_N, POWER_MAX_N

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "power_plan_vectors.json").read_text())


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


RECORDED = GOLDEN["measured"]["device_against_host"]  # rel_tol = 4 x the worst relative difference measured on an MI355X, abs_tol = 1e-13
REL_TOL, ABS_TOL = RECORDED["rel_tol"], RECORDED["abs_tol"]


def test_the_recorded_tolerance_is_the_one_the_guard_is_built_from():
    assert ABS_TOL == hp.DEVICE_ABS_TOL == 1e-13 and REL_TOL == 4.0 * RECORDED["worst_relative_difference"] <= hp.DEVICE_REL_TOL < 1e-13
    assert hp.GUARD >= (hp.HOST_REL_TOL + hp.HOST_ABS_TOL) + (hp.DEVICE_REL_TOL + hp.DEVICE_ABS_TOL)


def _close(got, want, what) -> float:
    """Every device value within the recorded tolerance of the host statement's; returns the worst relative difference seen among
    values above the absolute tolerance (printed by the callers before they assert anything else)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and (got >= 0.0).all() and (got <= 1.0).all(), what
    big = want > ABS_TOL
    worst = float((np.abs(got - want)[big] / np.maximum(got, want)[big]).max()) if big.any() else 0.0
    print(f"{what}: worst relative difference {worst:.3e}, worst absolute below abs_tol {float(np.abs(got - want)[~big].max()) if (~big).any() else 0.0:.3e}")
    for g, w in zip(got.tolist(), want.tolist()):
        assert math.isclose(g, w, rel_tol=REL_TOL, abs_tol=ABS_TOL), (what, g, w)
    return worst


def _shape_cells() -> np.ndarray:
    pairs = cases.Q_PRODUCTION + cases.Q_UNDERFLOW
    return hp.make_cells(np.repeat(cases.SHAPE_NS, len(pairs)), np.tile([p[0] for p in pairs], len(cases.SHAPE_NS)),
                         np.tile([p[1] for p in pairs], len(cases.SHAPE_NS)))


@pytest.fixture(scope="module")
def shape_reference():
    """The host statement on the shape cells, per alpha: computed once."""
    cells = _shape_cells()
    return cells, {alpha: hp.power_cells_host(cells, hp.critical_value(alpha)) for alpha in cases.ALPHAS}


@pytest.mark.parametrize("alpha", cases.ALPHAS, ids=["ordinary", "family_150", "family_5160"])
def test_cell_shapes_against_the_host_statement(eng, shape_reference, alpha):
    cells, want = shape_reference
    assert POWER_LDS_MAX_N in cells["n"] and POWER_LDS_MAX_N + 1 in cells["n"] and cells["n"].max() == 20001
    got = eng.score_power_scan(cells, alpha)
    _close(got, want[alpha], f"shapes at alpha {alpha:g}")
    t = eng.timing()
    assert 0.0 < t["play_ms"] == t["total_ms"]
    under = np.isin(cells["q_ab"], (0.01, 0.99))
    assert (got[under & (cells["n"] >= 255)] > 1.0 - 1e-9).all()  # rejection is certain while whole tails underflow


def test_full_scan_of_small_sizes(eng):
    n = np.repeat(np.arange(1, 301), len(cases.Q_PRODUCTION))
    cells = hp.make_cells(n, np.tile([q[0] for q in cases.Q_PRODUCTION], 300), np.tile([q[1] for q in cases.Q_PRODUCTION], 300))
    alpha = cases.ALPHAS[1]
    _close(eng.score_power_scan(cells, alpha), hp.power_cells_host(cells, hp.critical_value(alpha)), "n = 1 .. 300")


def test_results_do_not_depend_on_order_or_company(eng, shape_reference):
    cells, _ = shape_reference
    alpha = cases.ALPHAS[1]
    alone = eng.score_power_scan(cells, alpha)
    rng = np.random.default_rng(7)
    pick = np.concatenate([rng.permutation(len(cells)), rng.integers(0, len(cells), size=40)])  # shuffled, with duplicates
    mixed = eng.score_power_scan(cells[pick], alpha)
    assert mixed.tobytes() == alone[pick].tobytes()
    for at in (0, len(cells) - 1, int(np.flatnonzero(cells["n"] == POWER_LDS_MAX_N + 1)[0])):  # one cell: the grid of one workgroup
        assert eng.score_power_scan(cells[at:at + 1], alpha).tobytes() == alone[at:at + 1].tobytes()


def test_batch_sizes(eng):
    alpha = cases.ALPHAS[0]
    few = hp.make_cells(np.arange(1, 9).repeat(3), np.tile([q[0] for q in cases.Q_PRODUCTION], 8), np.tile([q[1] for q in cases.Q_PRODUCTION], 8))
    want = hp.power_cells_host(few, hp.critical_value(alpha))
    many = few[np.arange(70_000) % len(few)]
    got = eng.score_power_scan(many, alpha)
    _close(got[: len(few)], want, "n <= 8")
    assert got.tobytes() == got[: len(few)][np.arange(70_000) % len(few)].tobytes()  # 70 000 workgroups, every repeat the same bits
    assert eng.score_power_scan(np.zeros(0, dtype=POWER_CELL_DTYPE), alpha).shape == (0,)
    untouched = np.full(3, 7.0)
    assert eng._lib.fk_score_power_scan(eng._ctx, None, 0, 2.0, untouched.ctypes.data_as(C.c_void_p)) == 0 and (untouched == 7.0).all()


def test_workspace_and_table_reuse(eng, shape_reference):
    """After a call that grew the table and the workspace to n = 20001, a smaller call on the same context gives the bits of a fresh
    context; so does the large call again."""
    from farkle_ii_amd.backend import Engine

    cells, _ = shape_reference
    alpha = cases.ALPHAS[2]
    large = cells[cells["n"] == 20001]
    small = cells[cells["n"] <= POWER_LDS_MAX_N + 1]
    first = eng.score_power_scan(large, alpha)
    after = eng.score_power_scan(small, alpha)
    again = eng.score_power_scan(large, alpha)
    with Engine(0) as fresh:
        assert fresh.score_power_scan(small, alpha).tobytes() == after.tobytes()
        assert fresh.score_power_scan(large, alpha).tobytes() == first.tobytes() == again.tobytes()


def test_refusals(eng):
    from farkle_ii_amd.backend import FarkleHipError

    alpha = 0.05
    good_cells = hp.make_cells([5, 700], [0.53, 0.56], [0.47, 0.5])
    good = eng.score_power_scan(good_cells, alpha)

    def still_good():
        assert eng.score_power_scan(good_cells, alpha).tobytes() == good.tobytes()

    for n, q_ab, q_ba, match in ((0, 0.5, 0.5, "cell 1: n must be in"), (-3, 0.5, 0.5, "n must be in"), (POWER_MAX_N + 1, 0.5, 0.5, f"n must be in \\[1, {POWER_MAX_N}\\]"),
                                 (9, 0.0, 0.5, "strictly between 0 and 1"), (9, 0.5, 1.0, "strictly between 0 and 1"), (9, -0.1, 0.5, "strictly between"),
                                 (9, math.nan, 0.5, "strictly between"), (9, 0.5, math.inf, "strictly between")):
        bad = hp.make_cells([5, n], [0.53, q_ab], [0.47, q_ba])
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.score_power_scan(bad, alpha)
        assert err.value.code == FK_ERR_ARG, match
        still_good()
    lib, ctx = eng._lib, eng._ctx  # below the Python layer: the critical value, the count and the null pointers
    power = np.full(2, 7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for call, match in ((lambda: lib.fk_score_power_scan(ctx, p(good_cells), 2, 0.0, p(power)), "critical_value must be finite and positive"),
                        (lambda: lib.fk_score_power_scan(ctx, p(good_cells), 2, -1.96, p(power)), "critical_value must be finite and positive"),
                        (lambda: lib.fk_score_power_scan(ctx, p(good_cells), 2, math.inf, p(power)), "critical_value must be finite and positive"),
                        (lambda: lib.fk_score_power_scan(ctx, p(good_cells), 2, math.nan, p(power)), "critical_value must be finite and positive"),
                        (lambda: lib.fk_score_power_scan(ctx, p(good_cells), -1, 1.96, p(power)), "n_cells must not be negative"),
                        (lambda: lib.fk_score_power_scan(ctx, None, 2, 1.96, p(power)), "cells and power are required"),
                        (lambda: lib.fk_score_power_scan(ctx, p(good_cells), 2, 1.96, None), "cells and power are required")):
        assert call() == FK_ERR_ARG and match in lib.fk_last_error(ctx).decode()
        assert (power == 7.0).all()
        still_good()
    with pytest.raises(ValueError, match="alpha must be in"):
        eng.score_power_scan(good_cells, 1.0)


@pytest.mark.parametrize("name", list(cases.PLANS) + ["equality"])
def test_plans_on_the_hip_engine(eng, name):
    plan_name = cases.EQUALITY_PLAN if name == "equality" else name
    want = GOLDEN["plans"][plan_name]
    settings = cases.plan_settings(plan_name)
    if name == "equality":
        settings["target_power"] = cases.from_hex(want["worst_scenario_achieved_power"])
    plan = hp.plan_block_games(eng, **settings)
    print(f"{name}: block {plan['block_games']}, {plan['host_evaluations']} host evaluations, {len(plan['curve'])} sizes scanned")
    assert plan["block_games"] == want["block_games"] == cases.PLANS[plan_name][4]
    assert cases.hex_of(plan["worst_scenario_achieved_power"]) == want["worst_scenario_achieved_power"]
    assert cases.hex_of(plan["previous_equal_block_size_worst_power"]) == want["previous_equal_block_size_worst_power"]
    assert 1 <= plan["host_evaluations"] <= hp.MAX_HOST_EVALUATIONS
    at = plan["block_games"] - 1  # the device's own value at the plan: within the guard of the host statement's
    assert abs(plan["curve"][at, -1] - plan["worst_scenario_achieved_power"]) <= hp.GUARD
