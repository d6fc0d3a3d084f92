"""`farkle root-stability`: over two small `farkle run --performance-bootstrap` trees (two roots) the three frames of the two-root
stability stage's bootstrap families — on the stub engine (the NumPy host statement) and, on the MI355X, on the HIP engine, which
must write the same files; both equal to the host module called directly on the same matrices; and every refusal of the command."""
from __future__ import annotations

import shutil
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

KS = (2, 4, 5)
SEEDS = (42, 57)
SCREENING = ("  bootstrap_replicates: 60\n  delta_across_k: 0.02\n  candidate_contribution_size: 7\n"
             "  practical_delta_by_k: {2: 0.03, 4: 0.02, 5: 0.02}\n")
EXTRA = "robustness:\n  delta_seed_stability: 0.04\n  joint_discrepancy_alpha: 0.1\nk_aggregation:\n  method: declared-mapping\n  k_weights: {2: 0.5, 4: 0.25, 5: 0.25}\n"
FILES = ("root_bootstrap_top_n_inclusion", "root_discrepancies", "root_joint_discrepancy")


def _stub():
    import root_stability_engine_stub

    return root_stability_engine_stub.Engine(0)


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        stub = _stub()
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out", screening: str = SCREENING, extra: str = EXTRA) -> Path:
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 6")
    assert "interval_confidence: 0.95\n" in text
    text = text.replace("interval_confidence: 0.95\n", "interval_confidence: 0.95\n" + screening) + "\n" + extra
    path = tmp_path / f"{name}.yaml"
    path.write_text(text)
    return path


def _two_trees(tmp_path: Path):
    """Two `farkle run --performance-bootstrap` trees of different roots -> (config path, [results root a, results root b])."""
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    cfg_path = _config(tmp_path)
    roots = []
    for seed in SEEDS:
        main(["--config", str(cfg_path), "--set", f"sim.seed_list=[{seed}]", "run", "--performance-bootstrap"])
        cfg = load_app_config(cfg_path, seed_list_len=None)
        cfg.sim.seed_list = [seed]
        cfg.sim.populate_seed_list(1)
        assert all(cfg.performance_batch_matrix_path(k).exists() for k in KS)
        roots.append(cfg.results_root)
    return cfg_path, roots


def _read(directory: Path) -> dict:
    import pyarrow.parquet as pq

    return {name: pq.read_table(directory / "root_stability" / f"{name}.parquet") for name in FILES}


def _direct(roots) -> dict:
    """The host module called directly on the matrices of the two trees, on the stub engine."""
    from farkle_ii_amd import root_stability as rs

    paths = [root / "analysis" / "03_metrics" / "by_k" / f"{k}p" / "performance_batch_matrix.npy" for root in roots for k in KS]
    cells = rs.load_cells(paths, SEEDS, KS)
    return rs.root_stability_tables(_stub(), cells, 60, 7, {2: 0.03, 4: 0.02, 5: 0.02}, 0.02, 0.04, 0.1, "declared-mapping",
                                    {2: 0.5, 4: 0.25, 5: 0.25})


def test_farkle_root_stability_writes_the_three_frames(engine, tmp_path):
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import root_stability as rs
    from farkle_ii_amd.cli import main

    cfg_path, roots = _two_trees(tmp_path)
    out = tmp_path / "pair"
    main(["--config", str(cfg_path), "root-stability", "--root-results", str(roots[1]), "--root-results", str(roots[0]), "--out", str(out)])
    got = _read(out)
    want = _direct(roots)
    S = 80
    assert got["root_bootstrap_top_n_inclusion"].num_rows == 2 * S and got["root_discrepancies"].num_rows == 4 * S
    assert got["root_joint_discrepancy"].num_rows == 1
    for name in FILES:
        assert got[name].schema.equals(want[name].schema) and got[name].equals(want[name]), name
    assert got["root_discrepancies"].schema.equals(rs.discrepancy_schema())
    assert got["root_bootstrap_top_n_inclusion"].column("root_seed").to_pylist() == [42] * S + [57] * S  # roots ascending whatever the order given
    assert got["root_bootstrap_top_n_inclusion"].column("k_aggregation_method").to_pylist() == ["declared_k_weighted_mean"] * (2 * S)
    assert sum(got["root_bootstrap_top_n_inclusion"].column("bootstrap_top_n_inclusion_frequency").to_pylist()) == pytest.approx(14.0)
    summary = got["root_joint_discrepancy"].to_pylist()[0]
    assert (summary["root_a"], summary["root_b"], summary["bootstrap_replicates"]) == (42, 57, 60)
    assert summary["joint_reference_upper_tail_fraction"] == 0.1 and summary["joint_max_abs_standardized_reference_quantile"] > 0.0
    assert set(got["root_discrepancies"].column("stability_threshold").to_pylist()) == {0.04}
    # the same command on the stub engine writes the same files (on the stub parameter this repeats the run into another directory)
    eng_mod.set_engine(_stub())
    try:
        main(["--config", str(cfg_path), "root-stability", "--root-results", str(roots[0]), "--root-results", str(roots[1]),
              "--out", str(tmp_path / "pair_stub")])
    finally:
        eng_mod.set_engine(None)
    again = _read(tmp_path / "pair_stub")
    for name in FILES:
        assert again[name].equals(got[name]), name
    # without --out: roots_<a>_<b> beside the first results root
    eng_mod.set_engine(engine)
    main(["--config", str(cfg_path), "root-stability", "--root-results", str(roots[0]), "--root-results", str(roots[1])])
    assert _read(roots[0].parent / "roots_42_57")["root_discrepancies"].equals(got["root_discrepancies"])


def test_refusals_of_the_command(tmp_path):
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.performance_bootstrap import BatchMatrix

    eng_mod.set_engine(_stub())
    try:
        cfg_path, roots = _two_trees(tmp_path)
        a, b = (["--root-results", str(r)] for r in roots)
        out = ["--out", str(tmp_path / "refused")]

        def refused(match, *argv, config=cfg_path):
            with pytest.raises(ValueError, match=match):
                main(["--config", str(config), "root-stability", *argv, *out])
            assert not (tmp_path / "refused").exists()

        refused("exactly two roots", *a)                      # one root
        refused("exactly two roots", *a, *a)                  # equal directories
        refused("exactly two roots", *a, *b, *a)              # more than two
        copy = tmp_path / "copy_of_a"
        shutil.copytree(roots[0], copy)
        refused("both --root-results hold root 42", *a, "--root-results", str(copy))  # equal roots in different directories
        matrix = copy / "analysis" / "03_metrics" / "by_k" / "4p" / "performance_batch_matrix.npy"
        matrix.unlink()
        refused("missing: .*4p.performance_batch_matrix.npy", "--root-results", str(copy), *b)  # a missing cell
        # differing strategy support: root b's 4-player matrix without its last strategy column
        narrow = tmp_path / "narrow_b"
        shutil.copytree(roots[1], narrow)
        path = narrow / "analysis" / "03_metrics" / "by_k" / "4p" / "performance_batch_matrix.npy"
        m = BatchMatrix.load(path, 4)
        BatchMatrix(m.root_seed, 4, m.batch_ids, m.strategies[:-1], m.wins[:, :-1], m.exposures[:, :-1], m.completed[:, :-1],
                    m.safety[:, :-1]).save(path)
        refused("strategy support differs", *a, "--root-results", str(narrow))
        for screening, match in ((SCREENING.replace("  practical_delta_by_k: {2: 0.03, 4: 0.02, 5: 0.02}\n", ""), "practical_delta_by_k is required"),
                                 (SCREENING.replace("delta_across_k: 0.02", "delta_across_k: null"), "delta_across_k is required"),
                                 (SCREENING.replace("{2: 0.03, 4: 0.02, 5: 0.02}", "{2: 0.03, 4: 0.02}"), "practical_delta_by_k is required for every"),
                                 (SCREENING.replace("bootstrap_replicates: 60", "bootstrap_replicates: 0"), "bootstrap_replicates")):
            refused(match, *a, *b, config=_config(tmp_path, name="bad", screening=screening))
        refused("declared k weights", *a, *b, config=_config(tmp_path, name="bad", extra=EXTRA.replace("{2: 0.5, 4: 0.25, 5: 0.25}", "{2: 0.5, 4: 0.5}")))
        refused("joint_discrepancy_alpha", *a, *b, config=_config(tmp_path, name="bad", extra=EXTRA.replace("alpha: 0.1", "alpha: 1.5")))
    finally:
        eng_mod.set_engine(None)


def test_defaults_are_the_references(tmp_path):
    """Without the robustness / k_aggregation sections: alpha 0.05, seed stability 0.03, equal-k."""
    from farkle_ii_amd.config import load_app_config

    settings = load_app_config(_config(tmp_path, extra=""), seed_list_len=1).root_stability_settings()
    assert settings == {"delta_seed_stability": 0.03, "joint_discrepancy_alpha": 0.05, "k_aggregation_method": "equal-k", "declared_k_weights": None}
    stated = load_app_config(_config(tmp_path), seed_list_len=1).root_stability_settings()
    assert stated == {"delta_seed_stability": 0.04, "joint_discrepancy_alpha": 0.1, "k_aggregation_method": "declared-mapping",
                      "declared_k_weights": {2: 0.5, 4: 0.25, 5: 0.25}}
