"""The per-root diagnostics on the CPU: the host statement ``rr_root_diagnostics.diagnose`` against the literal restatement of the
reference's ``_root_specific_diagnostics`` (tests/rr_root_diagnostics_literal.py) on the families of tests/rr_root_diagnostics_cases.py;
``rd_decision`` and ``rd_agreement`` of csrc/fk_rr_root_diagnostics.h (built into tests/native/rr_root_diagnostics_host_check.hip
without a GPU) over the sign table; the frames' columns and dtypes."""
from __future__ import annotations

import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rr_inference_cases as ri_cases
import rr_inference_literal as lit
import rr_root_diagnostics_cases as cases
import rr_root_diagnostics_literal as rd_lit
from farkle_ii_amd import rr_inference as ri
from farkle_ii_amd import rr_root_diagnostics as rd

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "rr_root_diagnostics_host_check.hip"
ALPHA = cases.PARAMS["family_alpha"]


def _same(got: float, want) -> bool:  # NaN is the literal's None
    return math.isnan(got) if want is None else got == want


def against_the_literal(case: dict, seeds, interval_every: int = 1) -> None:
    """Everything equal — integers, flags, decisions, strings, d_ab, discrepancies, Holm positions; the ordinary bounds (of every
    ``interval_every``-th pair: the literal's brentq loop is slow) within half of BOUND_TOL."""
    host = case["host"]
    diagnostics, agreement = rd_lit.root_specific_diagnostics(case["n"], case["roots"], seeds, [case["target"]] * len(seeds),
                                                              [case["cap"]] * len(seeds), family_alpha=ALPHA,
                                                              min_candidate_completion_rate=cases.PARAMS["min_candidate_completion_rate"],
                                                              interval_every=interval_every)
    roots = host["roots"].tolist()
    n_roots, n_pairs = host["rows"].shape
    assert roots == sorted(int(s) for s in seeds) and len(diagnostics) == n_roots * n_pairs and len(agreement) == n_pairs
    for k, want in enumerate(diagnostics):  # sorted by (pair_id, root_seed)
        got = host["rows"][k % n_roots][k // n_roots]
        assert roots[k % n_roots] == want["root_seed"] and got["pair_id"] == want["pair_id"]
        assert (got["strategy_a"], got["strategy_b"]) == (want["strategy_a"], want["strategy_b"])
        for name in ("games_attempted", "games_completed", "games_safety_limit", "completion_game_rate"):
            assert got[name] == want[name], name
        viable = want["pair_inferentially_viable"]
        assert bool(got["flags"] & ri.FLAG_INFERENTIAL) == viable and bool(got["flags"] & ri.FLAG_OPERATIONAL) == want["pair_operationally_viable"]
        assert bool(got["flags"] & ri.FLAG_ELIGIBLE) == want["pair_claim_eligible"] and bool(got["flags"] & ri.FLAG_REJECT) == want["holm_reject"]
        assert bool(got["flags"] & ri.FLAG_REJECT_BEFORE) == want["holm_reject_before_viability"]
        for name in ("n_ab", "n_ba", "seat1_a_wins_ab", "seat1_b_wins_ba"):  # (the record holds them for every pair, the frame nulls them)
            assert want[name] is None or got[name] == want[name], name
        for name in ("q_ab", "q_ba", "d_ab", "score_null_proportion", "score_z", "score_p_value"):
            assert _same(got[name], want[name]), (name, want["pair_id"])
        assert got["holm_order"] == (want["holm_order"] or 0)
        assert _same(got["holm_adjusted_p"], None if math.isnan(want["holm_adjusted_p"]) else want["holm_adjusted_p"])
        assert rd.DIAGNOSTIC_DECISIONS[got["diagnostic_decision"]] == want["diagnostic_holm_decision"]
        for name in ("ordinary_d_low", "ordinary_d_high"):
            if want[name] is None:  # no test, or a pair whose interval the literal skipped
                assert math.isnan(got[name]) == (not viable)
            else:
                assert abs(got[name] - want[name]) <= 0.5 * lit.BOUND_TOL, (name, want["pair_id"])
    for got, want in zip(host["agreement"], agreement):
        assert (got["pair_id"], got["strategy_a"], got["strategy_b"]) == (want["pair_id"], want["strategy_a"], want["strategy_b"])
        assert roots[0] == want["root_a"] and (roots[1] if n_roots == 2 else None) == want["root_b"]
        for name in ("root_a_d_ab", "root_b_d_ab", "effect_discrepancy_a_minus_b", "absolute_effect_discrepancy"):
            assert _same(got[name], want[name]), (name, want["pair_id"])
        assert rd.DIAGNOSTIC_DECISIONS[got["root_a_decision"]] == want["root_a_diagnostic_holm_decision"]
        if n_roots == 2:
            assert rd.DIAGNOSTIC_DECISIONS[got["root_b_decision"]] == want["root_b_diagnostic_holm_decision"]
        else:
            assert got["root_b_decision"] == rd.DECISION_NONE
        available = bool(got["flags"] & rd.AGREE_AVAILABLE)
        assert available == want["agreement_available"]
        assert (bool(got["flags"] & rd.AGREE_DECISION) if available else None) == want["diagnostic_holm_decision_agreement"]
        assert (bool(got["flags"] & rd.AGREE_DIRECTION) if available else None) == want["effect_direction_agreement"]
        assert available or not got["flags"]
    # the summary and the maximum, from the literal's rows
    s = host["summary"]
    on = [a for a in agreement if a["agreement_available"]]
    assert s[0] == n_pairs and s[1] == len(on) and s[2] == sum(a["diagnostic_holm_decision_agreement"] for a in on)
    assert s[3] == sum(a["effect_direction_agreement"] for a in on)
    for r, root in enumerate(roots):
        mine = [d for d in diagnostics if d["root_seed"] == root]
        assert s[4 + 4 * r: 7 + 4 * r].tolist() == [sum(d["diagnostic_holm_decision"] == name for d in mine) for name in rd.DIAGNOSTIC_DECISIONS]
        assert s[7 + 4 * r] == sum(d["formal_test_performed"] for d in mine)
    assert (s[4 + 4 * n_roots:] == 0).all()
    want_max = max((a["absolute_effect_discrepancy"] for a in on), default=None)
    assert _same(host["max_abs_discrepancy"], want_max)
    frame = rd.agreement_frame(host["agreement"], roots)
    assert frame["interpretation"].tolist() == [a["interpretation"] for a in agreement]


def test_synthetic_family_against_the_literal():
    against_the_literal(cases.synthetic(), cases.SYNTHETIC_SEEDS)


def test_wide_family_against_the_literal():
    against_the_literal(cases.wide(), cases.WIDE_SEEDS, interval_every=997)


def test_one_root_and_a_seed_with_the_top_bit():
    n, roots, target, cap = ri_cases.synthetic_family()
    one = {"n": n, "roots": roots[:1], "target": target, "cap": cap,
           "host": rd.diagnose(n, roots[:1], [5], [target], [cap], **cases.PARAMS)}
    against_the_literal(one, [5])
    assert one["host"]["summary"][1:4].tolist() == [0, 0, 0] and math.isnan(one["host"]["max_abs_discrepancy"])
    big = (1 << 63) + 7
    top = {"n": n, "roots": roots, "target": target, "cap": cap,
           "host": rd.diagnose(n, roots, [big, 3], [target] * 2, [cap] * 2, **cases.PARAMS)}
    against_the_literal(top, [big, 3])
    assert top["host"]["roots"].tolist() == [3, big]
    for bad in ([], [1, 2, 3], [4, 4], [-1], [1 << 64]):
        with pytest.raises(ValueError):
            rd.diagnose(n, roots[: max(len(bad), 1)] if len(bad) <= 2 else roots + roots[:1], bad, [target] * len(bad), [cap] * len(bad), **cases.PARAMS)


def test_rows_slice_and_pair_range():
    case = cases.wide()
    full = case["host"]
    part = rd.diagnose(case["n"], case["roots"], case["seeds"], [case["target"]] * 2, [case["cap"]] * 2, rows=(12_345, 13_001),
                       intervals="bisection", **cases.PARAMS)
    assert part["rows"].tobytes() == np.ascontiguousarray(full["rows"][:, 12_345:13_001]).tobytes()
    assert part["agreement"].tobytes() == full["agreement"][12_345:13_001].tobytes() and np.array_equal(part["summary"], full["summary"])
    lo, hi = 1_003, 9_130  # a resident range inside the table: Holm's family is the range
    inside = rd.diagnose(case["n"], [st[lo:hi] for st in case["roots"]], case["seeds"], [case["target"]] * 2, [case["cap"]] * 2, pair_begin=lo,
                         intervals="bisection", **cases.PARAMS)
    assert inside["rows"]["pair_id"][0, 0] == lo and inside["rows"]["pair_id"][1, -1] == hi - 1 and inside["summary"][0] == hi - lo
    assert inside["rows"]["d_ab"].tobytes() == np.ascontiguousarray(full["rows"]["d_ab"][:, lo:hi]).tobytes()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("rr_root_diagnostics") / "rr_root_diagnostics_host_check"
    # host side only (the checker launches no kernel), as tests/test_rr_inference_host.py builds its checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True,
                   capture_output=True, text=True)
    return exe


def test_header_rules_over_the_sign_table(checker):
    """{-, -0.0, 0.0, +, NaN}^2 x decisions^2 (and holm_reject both ways) against the reference's expressions (:945-953, :1023-1050)."""
    effects = (-0.0125, -0.0, 0.0, 0.03125, math.nan)
    todo = [(a, da, b, db, reject) for a in effects for b in effects for da in range(3) for db in range(3) for reject in (0, 1)]
    text = "".join(f"{'nan' if math.isnan(a) else a.hex()} {da} {'nan' if math.isnan(b) else b.hex()} {db} {reject}\n" for a, da, b, db, reject in todo)
    out = subprocess.run([str(checker)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(todo) == 450
    for (a, da, b, db, reject), line in zip(todo, out):
        discrepancy, absolute, flags, decision = line.split()
        discrepancy, absolute, flags, decision = float.fromhex(discrepancy), float.fromhex(absolute), int(flags), int(decision)
        both = not math.isnan(a) and not math.isnan(b)
        if both:
            assert discrepancy.hex() == (a - b).hex() and absolute.hex() == abs(a - b).hex()
            want = rd.AGREE_AVAILABLE | (rd.AGREE_DECISION if da == db else 0) | (rd.AGREE_DIRECTION if int(np.sign(a)) == int(np.sign(b)) else 0)
        else:
            assert math.isnan(discrepancy) and math.isnan(absolute)
            want = 0
        assert flags == want, (a, da, b, db)
        names = str(np.where(bool(reject), np.where(a > 0.0, "diagnostic_advantage_a", "diagnostic_advantage_b"), "diagnostic_no_adjusted_rejection"))
        assert rd.DIAGNOSTIC_DECISIONS[decision] == names, (a, reject)
    zero = [f for (a, da, b, db, r), f in zip(todo, out) if a == 0.0 and b == 0.0 and da == db and r == 0]
    assert zero and all(int(f.split()[2]) == 7 for f in zero)  # -0.0 and 0.0 agree with each other, and with nothing else


def test_frames():
    import pandas as pd

    case = cases.synthetic()
    host = case["host"]
    ids = np.arange(100, 100 + 7 * case["n"], 7)
    frame = rd.root_pairs_frame(host["rows"], host["roots"], ids, family_alpha=ALPHA)
    assert tuple(frame.columns) == rd.ROOT_PAIR_COLUMNS and len(frame) == 132
    assert frame["root_seed"].tolist()[:4] == [11, 12, 11, 12] and frame["pair_id"].tolist()[:4] == [0, 0, 1, 1]  # sorted by (pair_id, root_seed)
    assert frame["root_seed"].dtype == np.uint64 and frame["strategy_a"].tolist()[:2] == [100, 100] and frame["strategy_b"].tolist()[:2] == [107, 107]
    for name in ("n_ab", "n_ba", "seat1_a_wins_ab", "seat1_b_wins_ba", "holm_order"):
        assert frame[name].dtype == pd.Int64Dtype(), name
    for name in ("pair_inferentially_viable", "pair_operationally_viable", "pair_claim_eligible", "holm_reject"):
        assert frame[name].dtype == bool, name
    for name in ("completion_game_rate", "q_ab", "q_ba", "d_ab", "score_null_proportion", "score_z", "score_p_value", "ordinary_alpha",
                 "ordinary_d_low", "ordinary_d_high", "holm_adjusted_p"):
        assert frame[name].dtype == np.float64, name
    short = frame[frame["pair_id"] == ri_cases._pairs(case["n"]).index(ri_cases.SHORT)]
    assert short["n_ab"].isna().all() and short["holm_order"].isna().all() and (short["completion_status"] == "unresolved_nonviable").all()
    assert set(frame["diagnostic_holm_decision"]) == set(rd.DIAGNOSTIC_DECISIONS) and (frame["inference_role"] == rd.INFERENCE_ROLE).all()
    assert (frame["ordinary_alpha"] == ALPHA).all()

    agree = rd.agreement_frame(host["agreement"], host["roots"], ids)
    assert tuple(agree.columns) == rd.AGREEMENT_COLUMNS and len(agree) == 66
    assert (agree["root_a"] == 11).all() and (agree["root_b"] == 12).all() and agree["root_a"].dtype == np.uint64 and agree["root_b"].dtype == pd.UInt64Dtype()
    assert agree["diagnostic_holm_decision_agreement"].dtype == pd.BooleanDtype() and agree["effect_direction_agreement"].dtype == pd.BooleanDtype()
    assert agree["agreement_available"].dtype == bool and agree["agreement_available"].sum() == 65
    off = agree[~agree["agreement_available"]]
    assert off["diagnostic_holm_decision_agreement"].isna().all() and (off["interpretation"] == "unavailable_for_unresolved_nonviable_pair").all()
    assert (agree["effect_discrepancy_a_minus_b"].dropna() == (agree["root_a_d_ab"] - agree["root_b_d_ab"]).dropna()).all()

    n, roots, target, cap = ri_cases.synthetic_family()
    single = rd.diagnose(n, roots[:1], [9], [target], [cap], **cases.PARAMS)
    lone = rd.agreement_frame(single["agreement"], single["roots"], ids)
    assert lone["root_b"].isna().all() and lone["root_b_diagnostic_holm_decision"].isna().all() and not lone["agreement_available"].any()
    assert (lone["interpretation"] == "single_root_diagnostic_no_cross_root_stability_claim").all() and lone["root_b_d_ab"].isna().all()

    digest = rd.stability_summary(host["summary"])
    assert digest == {"available": True, "pair_count": 66, "diagnostic_decision_agreement_fraction": 61 / 65,
                      "effect_direction_agreement_fraction": 61 / 65, "interpretation": "fixed_root_reproducibility_not_root_population_inference"}
    assert rd.stability_summary(single["summary"])["available"] is False
    assert rd.stability_summary(single["summary"])["diagnostic_decision_agreement_fraction"] is None
