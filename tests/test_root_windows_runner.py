"""`farkle root-stability --diagnostics`: over two trees that hold the golden cases' batch matrices the command writes eleven files —
the eight diagnostic frames, equal to the reference's (tests/golden/root_stability_frames_vectors.json), beside the three of the
bootstrap families — on the stub engine (the NumPy host statements) and, on the MI355X, on the HIP engine; without the flag it
writes the three files of before."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import root_windows_cases as cases  # noqa: E402

THREE = ("root_bootstrap_top_n_inclusion", "root_discrepancies", "root_joint_discrepancy")
REPLICATES = 40


def _stub():
    import root_windows_engine_stub

    return root_windows_engine_stub.Engine(0)


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


def _config(tmp_path: Path, case: dict, extra: str = "") -> Path:
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / "unused"}"')
    assert "n_players_list: [2, 4, 5]" in text and "interval_confidence: 0.95\n" in text
    text = text.replace("n_players_list: [2, 4, 5]", f"n_players_list: {case['required_k']}")
    practical = ", ".join(f"{k}: {v}" for k, v in case["practical_delta_by_k"].items())
    screening = (f"  bootstrap_replicates: {REPLICATES}\n  delta_across_k: {case['delta_across_k']}\n"
                 f"  candidate_contribution_size: {case['candidate_contribution_size']}\n  practical_delta_by_k: {{{practical}}}\n"
                 f"  controls: {case['controls']}\n")
    text = text.replace("interval_confidence: 0.95\n", "interval_confidence: 0.95\n" + screening)
    text += (f"\nrobustness:\n  delta_seed_stability: {case['delta_seed_stability']}\n  matched_count_fractions: {case['matched_count_fractions']}\n"
             f"resources:\n  stage_batch_bytes: {{performance: {case['stage_batch_bytes']}}}\n")
    if case["k_weights"] is not None:
        weights = ", ".join(f"{k}: {v}" for k, v in case["k_weights"].items())
        text += f"k_aggregation:\n  method: {case['k_aggregation_method']}\n  k_weights: {{{weights}}}\n"
    path = tmp_path / "stage.yaml"
    path.write_text(text + extra)
    return path


def _trees(tmp_path: Path, case: dict) -> list:
    cells = cases.golden_cells(case)
    roots = []
    for root in cells.roots:
        directory = tmp_path / f"results_seed_{root}"
        for k in cells.required_k:
            cells.matrices[(root, k)].save(directory / "analysis" / "03_metrics" / "by_k" / f"{k}p" / "performance_batch_matrix.npy")
        roots.append(directory)
    return roots


def _read(directory: Path) -> dict:
    import pyarrow.parquet as pq

    return {path.stem: pq.read_table(path) for path in sorted((directory / "root_stability").glob("*.parquet"))}


@pytest.mark.parametrize("name", cases.GOLDEN_NAMES)
def test_diagnostics_write_eleven_files_that_equal_the_reference_s(engine, tmp_path, name):
    """Through the runner with the fixture's ``np.dot`` columns fed in: the eight frames are the reference's, the three of the
    bootstrap families are those of the stage without the flag (their estimates now come from the window call)."""
    from farkle_ii_amd import root_stability as rs
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    case = cases.golden_case(name)
    cfg = load_app_config(_config(tmp_path, case), seed_list_len=1)
    roots = _trees(tmp_path, case)
    written = runner.run_root_stability(cfg, roots, out=tmp_path / "pair", diagnostics=True, across_k=cases.golden_across(case))
    got = _read(tmp_path / "pair")
    assert sorted(got) == sorted(written) == sorted(list(case["frames"]) + list(THREE)) and len(got) == 10 + len(case["required_k"])
    for frame, recorded in case["frames"].items():
        cases.assert_same_table(got[frame], cases.golden_table(recorded), (name, frame))
    settings = cases.golden_settings(case)
    want = rs.root_stability_tables(_stub(), cases.golden_cells(case), REPLICATES, settings["candidate_contribution_size"],
                                    settings["practical_delta_by_k"], settings["delta_across_k"], settings["delta_seed_stability"], 0.05,
                                    settings["k_aggregation_method"], settings["declared_k_weights"], across_k=cases.golden_across(case)["full"])
    if name != "chunks_3_3_1":  # (there the window call's chunks give other bits than the one-chunk chain: that is the case's point)
        for frame in THREE:
            cases.assert_same_table(got[frame], want[frame], (name, frame))


def test_the_command_knows_the_flag(engine, tmp_path):
    """``farkle root-stability --diagnostics`` writes the eleven files, equal to the module called directly; without the flag the
    three files, which hold what they held before."""
    from farkle_ii_amd import root_stability as rs
    from farkle_ii_amd.cli import main

    case = cases.golden_case("k23_unequal")
    cfg_path, roots = _config(tmp_path, case), _trees(tmp_path, case)
    arguments = ["--config", str(cfg_path), "root-stability", "--root-results", str(roots[1]), "--root-results", str(roots[0])]
    main(arguments + ["--out", str(tmp_path / "with"), "--diagnostics"])
    main(arguments + ["--out", str(tmp_path / "without")])
    with_flag, without = _read(tmp_path / "with"), _read(tmp_path / "without")
    assert sorted(without) == sorted(THREE) and len(with_flag) == 12
    settings = cases.golden_settings(case)
    direct = rs.root_stability_diagnostic_tables(_stub(), cases.golden_cells(case), REPLICATES, joint_discrepancy_alpha=0.05, **settings)
    assert sorted(direct) == sorted(with_flag)
    for frame, table in direct.items():
        cases.assert_same_table(with_flag[frame], table, frame)
    before = rs.root_stability_tables(_stub(), cases.golden_cells(case), REPLICATES, settings["candidate_contribution_size"],
                                      settings["practical_delta_by_k"], settings["delta_across_k"], settings["delta_seed_stability"], 0.05,
                                      settings["k_aggregation_method"], settings["declared_k_weights"])
    for frame in THREE:
        cases.assert_same_table(without[frame], before[frame], frame)
        cases.assert_same_table(with_flag[frame], before[frame], frame)  # one chunk per window here: the same estimates either way


def test_settings_and_their_refusals(tmp_path):
    from farkle_ii_amd.config import load_app_config

    case = cases.golden_case("k23_unequal")
    settings = load_app_config(_config(tmp_path, case), seed_list_len=1).root_stability_diagnostic_settings()
    assert settings == {"matched_count_fractions": (0.25, 0.5, 0.75, 1.0), "stage_batch_bytes": 16 << 20, "controls": [8, 41, 8]}
    chunked = load_app_config(_config(tmp_path, cases.golden_case("chunks_3_3_1")), seed_list_len=1).root_stability_diagnostic_settings()
    assert chunked["stage_batch_bytes"] == 57 * 12 * 3
    text = _config(tmp_path, case).read_text()
    plain = tmp_path / "plain.yaml"
    plain.write_text(text[:text.index("\nrobustness:")] + "\n")
    assert load_app_config(plain, seed_list_len=1).root_stability_diagnostic_settings()["matched_count_fractions"] == (0.25, 0.5, 0.75, 1.0)
    assert load_app_config(plain, seed_list_len=1).root_stability_diagnostic_settings()["stage_batch_bytes"] == 16 << 20
    for fractions in ("[0.5, 0.25, 1.0]", "[0.5, 0.5, 1.0]", "[0.0, 1.0]", "[0.5, 1.5]", "[0.25, 0.5]", "[]"):
        bad = tmp_path / "bad.yaml"
        bad.write_text(text.replace(f"matched_count_fractions: {case['matched_count_fractions']}", f"matched_count_fractions: {fractions}"))
        with pytest.raises(ValueError, match="matched_count_fractions must be unique increasing values in \\(0, 1\\] ending at 1"):
            load_app_config(bad, seed_list_len=1).root_stability_diagnostic_settings()
    for budgets in ("{performance: 0}", "{performance: true}", "{}"):
        bad = tmp_path / "bad.yaml"
        bad.write_text(text.replace(f"{{performance: {case['stage_batch_bytes']}}}", budgets))
        with pytest.raises(ValueError, match="stage_batch_bytes must contain positive integer stage budgets"):
            load_app_config(bad, seed_list_len=1).root_stability_diagnostic_settings()
    fallback = tmp_path / "fallback.yaml"
    fallback.write_text(text.replace(f"{{performance: {case['stage_batch_bytes']}}}", "{analysis: 4096}"))
    assert load_app_config(fallback, seed_list_len=1).root_stability_diagnostic_settings()["stage_batch_bytes"] == 4096
