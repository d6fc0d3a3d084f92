"""Cases of the power-plan tests (test helper, not a conftest): the cells whose exact power tests/golden/power_plan_vectors.json records
from the reference (tools/gen_power_plan_golden.py), the boundary cases whose digests it records, the plans, and an engine whose scan is
the host statement."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from farkle_ii_amd import h2h_power as hp
from farkle_ii_amd.backend import POWER_LDS_MAX_N

SCENARIOS = (0.0, 0.03, 0.06)
FAMILY_ALPHA = 0.02
ALPHAS = (0.05, 0.02 / 11175, 0.02 / 13310220)  # ordinary; Bonferroni of 150 candidates; of the 5 160-strategy grid
Q_PRODUCTION = tuple(hp.scenario_probabilities(0.03, s) for s in SCENARIOS)
Q_UNDERFLOW = ((0.01, 0.99), (0.99, 0.01))  # whole tails underflow
# the sizes at which the kernel changes shape: below, at and above a wave and a workgroup; several chunks; the production sizes around
# the plan; the last size whose tails fit LDS and the first beyond; a size of the whole-grid family's order
SHAPE_NS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4380, 4382, POWER_LDS_MAX_N, POWER_LDS_MAX_N + 1, 20001)
SCAN_NS = tuple(range(1, 201))
BOUNDARY_DIGEST_NS = (1, 2, 3, 64, 600, 1023, 1024, 1025, 4380, 4382, 20001)

# name: candidates, roots, effect, target power, the block size the reference plans
PLANS = {"production": (150, 2, 0.03, 0.80, 2191), "four": (4, 1, 0.20, 0.80, 43), "six": (6, 2, 0.15, 0.80, 45), "three": (3, 1, 0.25, 0.90, 30)}
EQUALITY_PLAN = "four"  # the same plan with the reference's own worst power at its block size as the target

# the keys of the reference's plan dict that h2h_power_plan.json holds
DOCUMENT_KEYS = ("candidate_count", "unordered_pair_count", "root_seeds", "single_root_execution", "score_test_id", "power_method_id",
                 "h2h_method_version", "test_direction", "final_multiplicity_method", "planning_multiplicity_method", "family_alpha",
                 "alpha_per_pair", "target_power", "power_conditioning", "target_effect", "n_completed_required_per_root_order_block",
                 "n_completed_required_per_order_across_roots", "n_completed_required_per_pair", "total_completed_required",
                 "max_attempt_multiplier", "max_attempts_per_root_order_block", "maximum_total_attempts", "min_candidate_completion_rate",
                 "total_block_count", "worst_scenario_achieved_power", "previous_equal_block_size_worst_power", "power_validation")


def golden_cells() -> list[tuple[int, float, float, float]]:
    """``(n, q_ab, q_ba, alpha)`` of every recorded cell, in the file's order."""
    cells = [(n, q_ab, q_ba, alpha) for alpha in ALPHAS for n in SHAPE_NS for q_ab, q_ba in Q_PRODUCTION + Q_UNDERFLOW]
    cells += [(n, q_ab, q_ba, ALPHAS[1]) for n in SCAN_NS for q_ab, q_ba in Q_PRODUCTION]
    return cells


def plan_settings(name: str) -> dict:
    candidates, roots, effect, target, _ = PLANS[name]
    return dict(root_count=roots, effect=effect, scenarios=SCENARIOS, alpha_per_pair=FAMILY_ALPHA / (candidates * (candidates - 1) // 2),
                target_power=target)


def hex_of(value: float) -> str:
    return struct.pack(">d", float(value)).hex()


def from_hex(text: str) -> float:
    return struct.unpack(">d", bytes.fromhex(text))[0]


def boundary_digest(lower, upper) -> str:
    h = hashlib.sha256()
    for a in (lower, upper):
        h.update(np.ascontiguousarray(a, dtype="<i8").tobytes())
    return h.hexdigest()


class HostStatementEngine:
    """``score_power_scan`` by ``power_cells_host``; counts its calls and cells."""

    def __init__(self):
        self.calls, self.cells = 0, 0

    def score_power_scan(self, cells, alpha: float) -> np.ndarray:
        self.calls += 1
        self.cells += len(cells)
        return hp.power_cells_host(cells, hp.critical_value(alpha))
