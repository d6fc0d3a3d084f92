"""`farkle run --performance --performance-bootstrap`: per player count ``performance_by_k.parquet``, after the last one
``performance_across_k.parquet``, the descriptive screening frame and its report — against the frames built from the host statement over
the run's own batch matrices (the stub engine serves the stage with the host statement; on the MI355X the HIP engine computes it and
must write the same files), the ranks the agreement stage's membership loader takes, and the refusals."""
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

KS = (2, 4, 5)
PRACTICAL = {2: 0.05, 4: 0.04, 5: 0.03}
SCREENING = ("  bootstrap_replicates: 40\n  delta_across_k: 0.02\n  candidate_contribution_size: 7\n  controls: [3, 41]\n"
             "  mandatory_diagnostics: [5]\n  practical_delta_by_k: {2: 0.05, 4: 0.04, 5: 0.03}\n")


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import performance_engine_stub

        stub = performance_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out", screening: str = SCREENING) -> Path:
    """configs/fast_config.yaml with its results under tmp_path, a coarser screening resolution (fewer shuffles), six batches and the
    stage's settings."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 6")
    assert "interval_confidence: 0.95\n" in text
    text = text.replace("interval_confidence: 0.95\n", "interval_confidence: 0.95\n" + screening)
    path = tmp_path / f"{name}.yaml"
    path.write_text(text)
    return path


def test_farkle_run_performance_writes_the_frames_of_the_host_statement(engine, tmp_path):
    import pandas as pd
    import pyarrow.parquet as pq

    from farkle_ii_amd import performance as pf
    from farkle_ii_amd import performance_bootstrap as pb
    from farkle_ii_amd import structure_agreement as sa
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--performance", "--performance-bootstrap"])
    cfg = load_app_config(cfg_path, seed_list_len=1)
    metrics = cfg.results_root / "analysis" / "03_metrics"
    host = pf.HostEngine()
    tables, estimates = {}, {}
    for k in KS:
        assert cfg.performance_by_k_path(k) == metrics / "by_k" / f"{k}p" / "performance_by_k.parquet"
        matrix = pb.BatchMatrix.load(cfg.performance_batch_matrix_path(k), k)
        tables[k], estimates[k] = pf.by_k_frame(host, matrix, 0.2, PRACTICAL[k])
        got = pq.read_table(cfg.performance_by_k_path(k))
        assert got.schema.equals(pf.by_k_schema()) and got.equals(tables[k]) and got.num_rows == 80
    across, strategies, _ = pf.across_k_frame(host, estimates, KS, 0.02)
    assert cfg.performance_across_k_path() == metrics / "across_k" / "performance_across_k.parquet"
    got = pq.read_table(cfg.performance_across_k_path())
    assert got.schema.equals(pf.across_k_schema(False)) and got.equals(across) and len(strategies) == 80
    assert sum(got.column("maximin_leader").to_pylist()) == 1 and 1 <= sum(got.column("pareto_member").to_pylist()) <= 80
    bootstrap = pq.read_table(cfg.performance_bootstrap_path())
    want = pf.screening_frame(across, bootstrap, tables, KS, 7, 0.02, PRACTICAL, [3, 41], [5])
    assert cfg.screening_path() == cfg.results_root / "analysis" / "04_screening" / "across_k" / "descriptive_screening.parquet"
    screening = pq.read_table(cfg.screening_path())
    assert screening.schema.equals(want.schema) and screening.equals(want)
    assert screening.column("score_order_position").to_pylist() == list(range(1, 81))
    assert sum(screening.column("observed_top_n").to_pylist()) == 7 and sum(screening.column("declared_control").to_pylist()) == 2
    report = json.loads(cfg.screening_path("descriptive_screening.json").read_text())
    assert report == pf.screening_payload(want, KS) and report["strategy_count"] == 80 and report["player_counts"] == [2, 4, 5]
    # the rank the agreement stage asks the caller for: score_order_position, taken by its membership loader as it stands
    ranks = pf.win_rate_ranks(screening)
    top = [s for s, flag in zip(screening.column("strategy").to_pylist(), screening.column("observed_top_n").to_pylist()) if flag]
    frame = pd.DataFrame({"strategy": screening.column("strategy").to_pylist(),
                          "win_rate_rank": pd.array(screening.column("score_order_position").to_pylist(), dtype="Int64"),
                          "trueskill_rank": pd.array(screening.column("score_order_position").to_pylist(), dtype="Int64"),
                          "family_hash": "f" * 64, **{flag: screening.column("observed_top_n").to_pylist() for flag in sa.MEMBERSHIP_FLAGS}})
    membership = sa.membership_from_frame(frame, sorted(top))
    assert membership["win_rate_rank"].tolist() == [ranks[s] for s in sorted(top)] and sorted(membership["win_rate_rank"].tolist()) == list(range(1, 8))


def test_performance_alone_and_refusals(tmp_path):
    import performance_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    eng_mod.set_engine(performance_engine_stub.Engine(0))
    try:
        for screening, match in ((SCREENING.replace("delta_across_k: 0.02", "delta_across_k: null"), "delta_across_k must be explicitly configured"),
                                 (SCREENING.replace("  practical_delta_by_k: {2: 0.05, 4: 0.04, 5: 0.03}\n", ""), "practical_delta_by_k must explicitly cover"),
                                 (SCREENING.replace("{2: 0.05, 4: 0.04, 5: 0.03}", "{2: 0.05, 4: 0.04}"), "keys must match sim.n_players_list"),
                                 (SCREENING.replace("5: 0.03}", "5: 0.0}"), "practical thresholds must be positive")):
            bad = _config(tmp_path, name="bad", screening=screening)
            with pytest.raises(ValueError, match=match):
                main(["--config", str(bad), "run", "--performance", "--force"])
            assert not load_app_config(bad, seed_list_len=1).n_dir(2).exists()  # refused before anything played
        alone = _config(tmp_path, name="alone")  # without the bootstrap: the estimates, no screening frame
        main(["--config", str(alone), "run", "--performance"])
        cfg = load_app_config(alone, seed_list_len=1)
        assert all(cfg.performance_by_k_path(k).exists() and cfg.performance_batch_matrix_path(k).exists() for k in KS)
        assert cfg.performance_across_k_path().exists() and not cfg.screening_path().exists() and not cfg.performance_bootstrap_path().exists()
        plain = _config(tmp_path, name="plain")  # a run already complete without the matrices: they need every batch of it
        main(["--config", str(plain), "run"])
        with pytest.raises(ValueError, match="--force"):
            main(["--config", str(plain), "run", "--performance"])
    finally:
        eng_mod.set_engine(None)
