"""`farkle round-robin --inference --agreement --candidate-membership FILE` on the CPU stub engine (tests/agreement_engine_stub.py) and
on the HIP engine (MI355X): the two artifacts it writes equal the host statements (``farkle_ii_amd.structure_agreement``) over the
decision classes the same run wrote; the combination with ``--root-diagnostics``; one root; the pairs left out, and the report saying
so, when not every pair's row comes to the host; and what the options refuse."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from test_rr_inference_runner import _base, _config, _family  # noqa: E402  (the same family and settings)

AGREEMENT_FILES = ["agreement_summary.json", "selection_conditioned_pairs.parquet"]
INFERENCE_FILES = ["round_robin.json", "round_robin_inference_pairs.parquet", "round_robin_inference_strategies.parquet", "round_robin_strategies.parquet"]
ROOT_FILES = ["root_decision_agreement.parquet", "root_pairwise_diagnostics.parquet"]
FAMILY_HASH = "runner-test-family"


@pytest.fixture(params=["host-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    eng_mod.set_engine(None)
    if request.param == "host-stub":
        import agreement_engine_stub

        eng_mod.set_engine(agreement_engine_stub.Engine(0))
    yield request.param
    eng_mod.set_engine(None)


def _membership(ids, tmp_path: Path, **changes):
    """A candidate membership whose final family is ``ids``: a scored population of the finalists and twelve others, one finalist
    without a TrueSkill rank, one of the others without a win-rate rank."""
    import pandas as pd

    rng = np.random.default_rng(11)
    everyone = np.array(sorted(set(ids) | {100_000 + k for k in range(12)}), dtype=np.int64)
    m = len(everyone)
    win = (1 + rng.permutation(m)).astype(np.float64)
    ts = (1 + np.argsort(np.argsort(win + rng.normal(0.0, 4.0, size=m)))).astype(np.float64)
    final = np.isin(everyone, ids)
    ts[np.flatnonzero(final)[2]] = np.nan
    win[np.flatnonzero(~final)[0]] = np.nan
    flags = {name: rng.random(m) < 0.5 for name in ("iw", "it", "fw", "ft", "control", "diagnostic")}
    frame = pd.DataFrame({
        "strategy": pd.array(everyone, dtype="Int32"), "win_rate_rank": pd.array(win, dtype="Int64"), "trueskill_rank": pd.array(ts, dtype="Int64"),
        "scored_by_both_methods": ~np.isnan(win) & ~np.isnan(ts), "initial_win_rate_contribution": flags["iw"],
        "initial_trueskill_contribution": flags["it"], "final_win_rate_contribution": flags["fw"] & final,
        "final_trueskill_contribution": flags["ft"] & final, "final_shared_contribution": flags["fw"] & flags["ft"] & final,
        "configured_control": flags["control"], "mandatory_diagnostic": flags["diagnostic"], "final_family": final, "family_hash": FAMILY_HASH,
    })
    for column, value in changes.items():
        frame[column] = value
    path = tmp_path / f"candidate_family_{'_'.join(changes) or 'good'}.parquet"
    frame.to_parquet(path)
    return path


def _host(out: Path, ids, membership_path: Path) -> dict:
    """The host statements over the decision classes this run wrote."""
    import pandas as pd

    from farkle_ii_amd import rr_inference as ri
    from farkle_ii_amd import structure_agreement as sa

    pairs = pd.read_parquet(out / "round_robin_inference_pairs.parquet")
    cls = np.array([ri.DECISION_CLASSES.index(c) for c in pairs["decision_class"]], dtype=np.uint8)
    membership = sa.read_membership(membership_path, ids)
    codes = sa.pair_codes(len(ids), cls, membership["win_rate_rank"], membership["trueskill_rank"])
    return {"membership": membership, "cls": cls, "codes": codes, "counts": sa.pair_counts(codes, cls),
            "concordance": sa.concordance_counts(*sa.scored_population(membership))}


def test_agreement_command_writes_the_host_statements(engine, tmp_path):
    import pandas as pd

    import dominance_cases
    from farkle_ii_amd import structure_agreement as sa
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    membership_path = _membership(ids, tmp_path)
    out = tmp_path / "rr"
    args = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--inference", "--agreement", "--candidate-membership", str(membership_path), "--out", str(out)]
    # two roots, with the per-root diagnostics
    main([*args, "--root-diagnostics"])
    assert sorted(f.name for f in out.iterdir()) == sorted(AGREEMENT_FILES + INFERENCE_FILES + ROOT_FILES)
    host = _host(out, ids, membership_path)
    report = json.loads((out / "round_robin.json").read_text())
    block = report["agreement"]
    assert block["pairs_written"] is True and set(AGREEMENT_FILES) <= set(report["files"]) and block["execution_scope"] == "root_pair"
    assert [block["counts"][name] for name in sa.COUNT_NAMES] == host["counts"].tolist() and block["counts"]["pairs"] == 28
    assert [block["concordance"][name] for name in sa.CONCORDANCE_NAMES] == host["concordance"].tolist()
    assert block["scored_population"] == 18 and block["family_hash"] == FAMILY_HASH
    stability = report["root_diagnostics"]["root_specific_h2h_stability"]
    summary = json.loads((out / "agreement_summary.json").read_text())
    assert summary == sa.summary(host["membership"], host["counts"], host["concordance"], stability, "root_pair")
    assert summary["root_specific_h2h_stability"]["pair_count"] == 28 and summary["admission_counts"]["final_family"] == 8
    assert summary["rank_agreement"]["kendall"] is not None and summary["common_scored_population_count"] == 18
    got, want = pd.read_parquet(out / "selection_conditioned_pairs.parquet"), sa.pairs_frame(host["codes"], host["cls"], ids, FAMILY_HASH)
    assert dominance_cases.frame_records(got)["rows"] == dominance_cases.frame_records(want)["rows"] and list(got.columns) == list(sa.PAIR_COLUMNS)
    assert host["counts"][1] > 0 and host["counts"][7] > 0  # directed pairs with a win-rate preference: the fractions are not empty
    # a slice of the rows: no pair table, and the report says so; no diagnostics: no stability block; with the dominance digest
    main([*args, "--dominance", "--rows", "5:9", "--force"])
    report = json.loads((out / "round_robin.json").read_text())
    assert report["agreement"]["pairs_written"] is False and "pairs_omitted" in report["agreement"]
    assert "selection_conditioned_pairs.parquet" not in report["files"] and "dominance_summary.json" in report["files"]
    assert report["agreement"]["counts"] == block["counts"]
    again = json.loads((out / "agreement_summary.json").read_text())
    assert again["root_specific_h2h_stability"] is None and {**again, "root_specific_h2h_stability": stability} == summary


def test_agreement_command_on_one_root(engine, tmp_path):
    from farkle_ii_amd import structure_agreement as sa
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    membership_path = _membership(ids, tmp_path)
    out = tmp_path / "rr"
    base = _base(cfg_path)
    at = base.index("round-robin")
    main([*base[:at], "--set", "sim.seed_list=[42]", *base[at:], "--strategy-ids", str(ids_file), "--inference", "--agreement", "--candidate-membership",
          str(membership_path), "--out", str(out)])
    host = _host(out, ids, membership_path)
    summary = json.loads((out / "agreement_summary.json").read_text())
    assert summary == sa.summary(host["membership"], host["counts"], host["concordance"], None, "single_root")
    assert summary["execution_scope"] == "single_root" and json.loads((out / "round_robin.json").read_text())["roots"] == [42]


def test_agreement_option_refusals(tmp_path):
    """Refused while reading the command line, the configuration and the membership: no engine is asked for."""
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    good = _membership(ids, tmp_path)
    base = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--out", str(tmp_path / "never")]
    with pytest.raises(SystemExit, match="--agreement belongs to --inference"):
        main([*base, "--agreement", "--candidate-membership", str(good)])
    with pytest.raises(SystemExit, match="--agreement needs --candidate-membership"):
        main([*base, "--inference", "--agreement"])
    with pytest.raises(SystemExit, match="--candidate-membership belongs to --agreement"):
        main([*base, "--inference", "--candidate-membership", str(good)])
    with pytest.raises(SystemExit, match=r"--agreement needs every pair of the table, --pairs plays \[4, 20\) of 28"):
        main([*base, "--inference", "--agreement", "--candidate-membership", str(good), "--pairs", "4:20"])
    at = base.index("round-robin")
    with pytest.raises(SystemExit, match="--agreement runs on one or two roots, got 3"):
        main([*base[:at], "--set", "sim.seed_list=[1, 2, 3]", *base[at:], "--inference", "--agreement", "--candidate-membership", str(good)])
    for changes, match in ((dict(final_family=True), "H2H inference finalist support differs from candidate provenance"),
                           (dict(family_hash=[f"h{k % 2}" for k in range(20)]), "candidate provenance must contain one final family hash"),
                           (dict(win_rate_rank=-1), "win_rate_rank must be a positive integer below")):
        with pytest.raises(SystemExit, match=match):
            main([*base, "--inference", "--agreement", "--candidate-membership", str(_membership(ids, tmp_path, **changes))])
    assert not (tmp_path / "never").exists()
