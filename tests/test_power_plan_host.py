"""The power plan on the CPU: ``pp_boundaries`` of csrc/fk_power_plan.h (built into tests/native/power_plan_host_check.hip without a
GPU) against ``h2h_power.boundaries`` integer for integer; ``boundaries``, ``score_test_power``, ``power_grid`` and the plans against
the reference's own results (tests/golden/power_plan_vectors.json, recorded by tools/gen_power_plan_golden.py), the exact statement bit
for bit and ``power_cells_host`` within the recorded tolerance; ``plan_block_games`` on an engine whose scan is the host statement;
the refusals of the search and of the configuration."""
from __future__ import annotations

import json
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import power_plan_cases as cases
from farkle_ii_amd import h2h_power as hp
from farkle_ii_amd.backend import POWER_CELL_DTYPE, POWER_LDS_MAX_N, POWER_MAX_N

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "power_plan_host_check.hip"
GOLDEN = json.loads((ROOT / "tests" / "golden" / "power_plan_vectors.json").read_text())
HEADER_CODE = (ROOT / "include" / "farkle_hip.h").read_text()


def test_the_golden_file_holds_every_case_and_is_small():
    assert GOLDEN["cells"]["count"] == len(GOLDEN["cells"]["power"]) == len(cases.golden_cells())
    assert sorted(GOLDEN["plans"]) == sorted(cases.PLANS) and len(GOLDEN["power_grid"]) == 6
    assert len(GOLDEN["boundaries"]) == len(cases.ALPHAS) * len(cases.BOUNDARY_DIGEST_NS)
    assert (ROOT / "tests" / "golden" / "power_plan_vectors.json").stat().st_size < 100_000
    assert {name: GOLDEN["plans"][name]["block_games"] for name in cases.PLANS} == {name: p[4] for name, p in cases.PLANS.items()}


def test_the_cell_layout_and_the_constants_are_the_header_s(tmp_path):
    """``fk_power_cell`` is declared with a tag, so the layout check of tests/test_abi_cpu.py does not see it: the same check here."""
    assert f"#define FK_POWER_MAX_N {POWER_MAX_N}\n" in HEADER_CODE and f"#define FK_POWER_LDS_MAX_N {POWER_LDS_MAX_N}\n" in HEADER_CODE
    fields = POWER_CELL_DTYPE.names
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "farkle_hip.h"', "int main() {", '    std::printf("%zu\\n", sizeof(fk_power_cell));']
    lines += [f'    std::printf("%zu %zu\\n", offsetof(fk_power_cell, {f}), sizeof(((fk_power_cell *)0)->{f}));' for f in fields]
    source = tmp_path / "power_cell_layout.hip"
    source.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = tmp_path / "power_cell_layout"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I", str(ROOT / "include"), "-o", str(exe), str(source)],
                   check=True, capture_output=True, text=True)
    out = [int(w) for w in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    assert out[0] == POWER_CELL_DTYPE.itemsize == 24
    assert list(zip(out[1::2], out[2::2])) == [(POWER_CELL_DTYPE.fields[f][1], POWER_CELL_DTYPE.fields[f][0].itemsize) for f in fields]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("power_plan") / "power_plan_host_check"
    # host side only (the checker launches no kernel), as tests/test_rr_inference_host.py builds its checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True, capture_output=True,
                   text=True)
    return exe


def test_header_boundaries_equal_numpy_integer_for_integer(checker):
    """Every c1 of every n in 1 .. 600 and of the sizes around the chunk edges, the production plan and the whole-grid family, at the
    ordinary alpha and at the two Bonferroni alphas."""
    sizes = list(range(1, 601)) + [1023, 1024, 1025, 4380, 4382, 20001]
    for alpha in cases.ALPHAS:
        critical = hp.critical_value(alpha)
        text = "".join(f"{n} {(critical ** 2).hex()}\n" for n in sizes)
        raw = subprocess.run([str(checker)], input=text.encode(), capture_output=True, timeout=120, check=True).stdout
        got = np.frombuffer(raw, dtype="<i4")
        assert len(got) == 2 * sum(n + 1 for n in sizes)
        at = 0
        for n in sizes:
            lower, upper = hp.boundaries(n, critical)
            assert np.array_equal(got[at:at + n + 1], lower) and np.array_equal(got[at + n + 1:at + 2 * (n + 1)], upper), (n, alpha)
            at += 2 * (n + 1)
            assert lower[0] == -1 and upper[n] == n + 1 and lower.min() >= -1 and lower.max() <= n and upper.min() >= 0 and upper.max() <= n + 1


def test_boundary_digests_equal_the_reference_s():
    for alpha in cases.ALPHAS:
        for n in cases.BOUNDARY_DIGEST_NS:
            assert cases.boundary_digest(*hp.boundaries(n, hp.critical_value(alpha))) == GOLDEN["boundaries"][f"{n}@{cases.hex_of(alpha)}"], (n, alpha)


def test_boundaries_are_the_rejection_rule():
    """The closed form against the score rule itself, count by count, at sizes small enough to enumerate."""
    for alpha in cases.ALPHAS:
        critical = hp.critical_value(alpha)
        for n in (1, 2, 7, 40):
            lower, upper = hp.boundaries(n, critical)
            for c1 in range(n + 1):
                for c2 in range(n + 1):
                    pooled = (c1 + c2) / (2.0 * n)
                    variance = pooled * (1.0 - pooled) * (2.0 / n)
                    rejects = abs((c1 - c2) / n / math.sqrt(variance)) > critical if variance > 0.0 else c1 != c2
                    assert rejects == (c2 <= lower[c1] or c2 >= upper[c1]), (n, alpha, c1, c2)


def test_score_test_power_is_the_reference_bit_for_bit():
    got = [cases.hex_of(hp.score_test_power(*cell)) for cell in cases.golden_cells()]
    assert got == GOLDEN["cells"]["power"]


def test_power_cells_host_within_the_recorded_tolerance():
    """``rel_tol`` is 4 x the worst relative difference the generator measured over these same cells; ``abs_tol`` the reference's 1e-13."""
    recorded = GOLDEN["measured"]["host_against_reference"]
    rel_tol, abs_tol = recorded["rel_tol"], recorded["abs_tol"]
    assert abs_tol == hp.HOST_ABS_TOL == 1e-13 and rel_tol == 4.0 * recorded["worst_relative_difference"] <= hp.HOST_REL_TOL < 1e-9
    assert hp.GUARD >= (hp.HOST_REL_TOL + hp.HOST_ABS_TOL) + (hp.DEVICE_REL_TOL + hp.DEVICE_ABS_TOL)
    cells = cases.golden_cells()
    want = [cases.from_hex(text) for text in GOLDEN["cells"]["power"]]
    worst = 0.0
    for alpha in cases.ALPHAS:
        at = [i for i, c in enumerate(cells) if c[3] == alpha]
        got = hp.power_cells_host(hp.make_cells(*(np.array([cells[i][k] for i in at]) for k in range(3))), hp.critical_value(alpha))
        for i, g in zip(at, got):
            assert math.isclose(g, want[i], rel_tol=rel_tol, abs_tol=abs_tol), (cells[i], g, want[i])
            if want[i] > abs_tol:
                worst = max(worst, abs(g - want[i]) / max(abs(g), abs(want[i])))
    print(f"power_cells_host against the reference: worst relative difference {worst:.3e} over {len(cells)} cells")
    assert any(0.0 < w < 1e-300 or w == 0.0 for w in want) and any(w > 0.999 for w in want)  # underflowing tails and saturated power both occur


@pytest.mark.parametrize("name", list(cases.PLANS) + ["equality"])
def test_plans_on_the_host_statement_engine(name):
    plan_name = cases.EQUALITY_PLAN if name == "equality" else name
    want = GOLDEN["plans"][plan_name]
    settings = cases.plan_settings(plan_name)
    if name == "equality":  # the target is the reference's own worst power at its block size: every device value near it is inside the guard
        settings["target_power"] = cases.from_hex(want["worst_scenario_achieved_power"])
    engine = cases.HostStatementEngine()
    plan = hp.plan_block_games(engine, **settings)
    assert plan["block_games"] == want["block_games"] == cases.PLANS[plan_name][4]
    assert cases.hex_of(plan["worst_scenario_achieved_power"]) == want["worst_scenario_achieved_power"]
    assert cases.hex_of(plan["previous_equal_block_size_worst_power"]) == want["previous_equal_block_size_worst_power"]
    assert 1 <= plan["host_evaluations"] <= hp.MAX_HOST_EVALUATIONS
    curve = plan["curve"]
    assert engine.calls == math.ceil(want["block_games"] / hp.DEFAULT_WINDOW) and engine.cells == len(curve) * len(cases.SCENARIOS)
    assert curve[:, 0].tolist() == list(range(1, len(curve) + 1)) and np.array_equal(curve[:, 1], curve[:, 0] * settings["root_count"])
    assert np.array_equal(curve[:, -1], curve[:, 2:-1].min(axis=1))
    worst = curve[: want["block_games"], -1]
    assert np.count_nonzero(np.diff(worst) < 0.0) >= 5  # the curve is not monotone: the scan is what finds the first crossing
    frame = hp.curve_frame(plan)
    assert list(frame.columns) == ["block_games", "games_per_order", "power_seat1_advantage_0", "power_seat1_advantage_0.03",
                                   "power_seat1_advantage_0.06", "worst_scenario_power"] and len(frame) == len(curve)


def test_power_grid_equals_the_reference_s_rows():
    candidates, roots, _, _, block = cases.PLANS["production"]
    rows = hp.power_grid(block, roots, (0.03, 0.04), cases.SCENARIOS, cases.plan_settings("production")["alpha_per_pair"])
    got = [{k: (cases.hex_of(v) if isinstance(v, float) else v) for k, v in row.items()} for row in rows]
    assert got == GOLDEN["power_grid"]


def test_plan_document_holds_the_reference_s_keys():
    from farkle_ii_amd.config import AppConfig

    cfg = AppConfig()
    cfg.opaque["head2head"] = {"practical_delta": 0.2, "sensitivity_deltas": [0.2]}
    plan = hp.plan_from_config(cases.HostStatementEngine(), cfg.head2head, 4, [42])
    doc = hp.plan_document(plan, cfg.head2head, 2.0)
    assert json.loads(json.dumps(doc)) == doc
    assert sorted(doc) == sorted(cases.DOCUMENT_KEYS)
    assert (doc["candidate_count"], doc["unordered_pair_count"], doc["root_seeds"], doc["single_root_execution"]) == (4, 6, [42], True)
    assert (doc["n_completed_required_per_root_order_block"], doc["n_completed_required_per_order_across_roots"],
            doc["n_completed_required_per_pair"], doc["total_completed_required"]) == (43, 43, 86, 516)
    assert (doc["max_attempts_per_root_order_block"], doc["maximum_total_attempts"], doc["total_block_count"]) == (86, 1032, 12)
    assert doc["alpha_per_pair"] == 0.02 / 6 and doc["score_test_id"] == hp.SCORE_TEST_ID and doc["h2h_method_version"] == 2
    assert cases.hex_of(doc["worst_scenario_achieved_power"]) == GOLDEN["plans"]["four"]["worst_scenario_achieved_power"]
    assert [row["achieved_power"] for row in doc["power_validation"]] == [hp.score_test_power(43, *hp.scenario_probabilities(0.2, s), 0.02 / 6)
                                                                          for s in cases.SCENARIOS]
    assert min(row["achieved_power"] for row in doc["power_validation"]) == doc["worst_scenario_achieved_power"]




def test_large_sample_formula_is_close_to_the_exact_power_at_the_production_plan():
    q_ab, q_ba = hp.scenario_probabilities(0.03, 0.0)
    alpha = cases.plan_settings("production")["alpha_per_pair"]
    assert abs(hp.independent_score_planning_power(4382, q_ab, q_ba, alpha) - hp.score_test_power(4382, q_ab, q_ba, alpha)) < 5e-3


def test_search_refusals():
    settings = cases.plan_settings("four")
    with pytest.raises(hp.PowerPlanError, match=f"no block size up to {POWER_MAX_N}"):  # an effect too small for any size the entry takes
        hp.plan_block_games(NeverEngine(), **{**settings, "effect": 1e-6}, window=1 << 19)
    with pytest.raises(hp.PowerPlanError, match="more than 8 block sizes lie within"):  # a scan that cannot separate sizes from the target
        hp.plan_block_games(cases.HostStatementEngine(), **settings, guard=0.5)
    with pytest.raises(hp.PowerPlanError, match="more than 2 block sizes"):
        hp.plan_block_games(cases.HostStatementEngine(), **settings, guard=0.05, max_host_evaluations=2)
    for bad, message in ((dict(target_power=1.0), "target_power must be in"), (dict(alpha_per_pair=0.0), "alpha_per_pair must be in"),
                         (dict(root_count=0), "at least one root"), (dict(scenarios=()), "at least one root"),
                         (dict(effect=0.6), "gives no valid probabilities")):
        with pytest.raises(ValueError, match=message):
            hp.plan_block_games(cases.HostStatementEngine(), **{**settings, **bad})
    from farkle_ii_amd.config import Head2HeadInferenceConfig

    h2h = Head2HeadInferenceConfig(allow_single_root=False, practical_delta=0.2, sensitivity_deltas=(0.2,))
    with pytest.raises(ValueError, match="disabled by head2head.allow_single_root"):
        hp.plan_from_config(cases.HostStatementEngine(), h2h, 4, [42])
    with pytest.raises(ValueError, match="one or two distinct root seeds"):
        hp.plan_from_config(cases.HostStatementEngine(), h2h, 4, [42, 42])
    with pytest.raises(ValueError, match="at least two candidates"):
        hp.plan_from_config(cases.HostStatementEngine(), h2h, 1, [1, 2])


class NeverEngine:
    """A scan that reports no power anywhere: the search runs to its limit without a host evaluation."""

    def score_power_scan(self, cells, alpha):
        return np.zeros(len(cells))


def test_config_fields_defaults_and_validations():
    from farkle_ii_amd.config import AppConfig

    h = AppConfig().head2head
    assert (h.target_power, h.seat1_advantage_scenarios, h.sensitivity_deltas, h.allow_single_root) == (0.80, (0.0, 0.03, 0.06), (0.03, 0.04), True)

    def read(**section):
        cfg = AppConfig()
        cfg.opaque["head2head"] = section
        h2h = cfg.head2head
        h2h.check_plan()
        return h2h

    h = read(target_power="0.9", practical_delta=0.2, sensitivity_deltas="[0.2, 0.25]", seat1_advantage_scenarios=[0, 0.1], allow_single_root="false")
    assert (h.target_power, h.sensitivity_deltas, h.seat1_advantage_scenarios, h.allow_single_root) == (0.9, (0.2, 0.25), (0.0, 0.1), False)
    for section, message in ((dict(target_power=0.0), "target_power must be between 0 and 1"), (dict(target_power=1.0), "target_power must be between"),
                             (dict(target_power="high"), "target_power must be a number"),
                             (dict(sensitivity_deltas=[0.04]), "unique positive values containing the practical delta"),
                             (dict(sensitivity_deltas=[0.03, 0.03]), "unique positive values"), (dict(sensitivity_deltas=[0.03, -0.1]), "unique positive values"),
                             (dict(sensitivity_deltas=[]), "list of numbers that is not empty"), (dict(sensitivity_deltas=0.03), "list of numbers"),
                             (dict(seat1_advantage_scenarios=["a"]), "list of numbers"), (dict(allow_single_root=1), "must be true or false"),
                             (dict(family_alpha=1.0), "family_alpha must be between 0 and 1"), (dict(practical_delta=0.0), "practical_delta must be positive")):
        with pytest.raises(ValueError, match=message):
            read(**section)
