"""`farkle round-robin --inference` on the HIP engine (MI355X): the tables it writes equal the frame builders of
farkle_ii_amd/rr_inference.py over the host statement fed with the states of a plain round robin of the same configuration; and what
the option refuses, before any engine exists."""
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

ROOTS = [42, 43]
BLOCK_GAMES, MULTIPLIER, MAX_ATTEMPTS = 40, 1.5, 60
PICK = (5, 0, 33, 79, 12, 48, 61, 27)  # positions in the grid, in file order (the command sorts by id)
KNOBS = dict(family_alpha=0.05, practical_delta=0.02, delta_equivalence=0.3, min_candidate_completion_rate=0.9)


def _config(tmp_path: Path) -> Path:
    """configs/fast_config.yaml (an 80-strategy grid) with its results under tmp_path."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / "out"}"')
    path = tmp_path / "cfg.yaml"
    path.write_text(text)
    return path


def _base(cfg_path: Path) -> list[str]:
    sets = [f"sim.seed_list={ROOTS}", f"head2head.max_attempt_multiplier={MULTIPLIER}", *(f"head2head.{k}={v}" for k, v in KNOBS.items())]
    return ["--config", str(cfg_path), *(a for s in sets for a in ("--set", s)), "round-robin", "--block-games", str(BLOCK_GAMES)]


def _family(cfg_path: Path, tmp_path: Path):
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    cfg = load_app_config(cfg_path, seed_list_len=None)
    strategies, _ = runner._resolve_strategies(cfg, None)
    grid = sorted(strategies, key=lambda s: int(s.strategy_id))
    chosen = sorted((grid[p] for p in PICK), key=lambda s: int(s.strategy_id))
    ids_file = tmp_path / "family.txt"
    ids_file.write_text("".join(f"{int(grid[p].strategy_id)}\n" for p in PICK))
    return chosen, ids_file


@pytest.mark.gpu
def test_inference_command_writes_what_the_host_statement_states(tmp_path):
    import pandas as pd

    import rr_inference_cases as cases
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd import rr_inference as ri
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.strategies import pack_strategies

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    eng_mod.set_engine(None)
    try:
        out = tmp_path / "rr"
        main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--inference", "--out", str(out)])
        assert sorted(f.name for f in out.iterdir()) == ["round_robin.json", "round_robin_inference_pairs.parquet",
                                                         "round_robin_inference_strategies.parquet", "round_robin_strategies.parquet"]
        # a plain round robin of the same configuration, and the host statement over its states
        engine = eng_mod.get_engine()
        table = pack_strategies(chosen)
        summary = np.zeros((8, 8), dtype=np.int64)
        states = [engine.h2h_round_robin(table, root, BLOCK_GAMES, MAX_ATTEMPTS, summary=summary)[0] for root in ROOTS]
        host = ri.infer(8, ri.combine_counts(states, [BLOCK_GAMES] * 2, [MAX_ATTEMPTS] * 2), **KNOBS)
        cases.assert_margins(host, KNOBS["practical_delta"], KNOBS["delta_equivalence"], KNOBS["family_alpha"])
        want_pairs = ri.pairs_frame(host["rows"], ids, **KNOBS)
        got_pairs = pd.read_parquet(out / "round_robin_inference_pairs.parquet")
        assert list(got_pairs.columns) == list(want_pairs.columns) and len(got_pairs) == 28
        loose = {"ordinary_d_low", "ordinary_d_high", "simultaneous_d_low", "simultaneous_d_high", "score_p_value", "holm_adjusted_p"}
        exact = [c for c in want_pairs.columns if c not in loose]
        pd.testing.assert_frame_equal(got_pairs[exact], want_pairs[exact], check_dtype=False, check_exact=True)
        for name in sorted(loose - {"score_p_value", "holm_adjusted_p"}):  # the halved bounds, as tests/test_rr_inference_gpu.py holds them
            assert np.nanmax(np.abs(got_pairs[name].to_numpy() - want_pairs[name].to_numpy())) <= 1.25e-12
        tested = want_pairs["formal_test_performed"].to_numpy()
        z = np.abs(want_pairs["score_z"].to_numpy()[tested])
        for name in ("score_p_value", "holm_adjusted_p"):  # Holm's products and maxima carry the p-values' relative distance
            got, want = got_pairs[name].to_numpy()[tested], want_pairs[name].to_numpy()[tested]
            assert (np.abs(got - want) <= cases.p_value_bound(z).max() * want).all(), name
        got_strategies = pd.read_parquet(out / "round_robin_inference_strategies.parquet")
        pd.testing.assert_frame_equal(got_strategies, ri.strategies_frame(host["strategies"], ids, KNOBS["min_candidate_completion_rate"]),
                                      check_dtype=False, check_exact=True)
        pd.testing.assert_frame_equal(pd.read_parquet(out / "round_robin_strategies.parquet"), rr.strategies_frame(ids, summary),
                                      check_dtype=False, check_exact=True)
        report = json.loads((out / "round_robin.json").read_text())
        assert report["inference"]["class_counts"] == {name: int(v) for name, v in zip(ri.DECISION_CLASSES, host["class_counts"])}
        assert report["inference"]["family_pair_count"] == 28 and (report["inference"]["row_begin"], report["inference"]["row_end"]) == (0, 28)
        assert report["games_attempted"] == int(sum(int(st[:, :, 0].sum()) for st in states))
        assert report["games_completed"] == int(sum(int(st[:, :, 1].sum()) for st in states))
        # a slice of the rows
        main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--inference", "--rows", "5:9", "--out", str(out), "--force"])
        part = pd.read_parquet(out / "round_robin_inference_pairs.parquet")
        pd.testing.assert_frame_equal(part, got_pairs.iloc[5:9].reset_index(drop=True), check_exact=True)
    finally:
        eng_mod.set_engine(None)


def test_inference_option_refusals(tmp_path):
    """Refused while reading the command line and the configuration: no engine is asked for."""
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    _, ids_file = _family(cfg_path, tmp_path)
    base = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--out", str(tmp_path / "never")]
    with pytest.raises(SystemExit, match="--rows belongs to --inference"):
        main([*base, "--rows", "0:4"])
    with pytest.raises(SystemExit, match="--blocks needs the block states on the host"):
        main([*base, "--inference", "--blocks"])
    with pytest.raises(SystemExit, match=r"--rows takes BEGIN:END inside the played pair range \[4, 20\)"):
        main([*base, "--inference", "--pairs", "4:20", "--rows", "2:10"])
    with pytest.raises(SystemExit, match="--rows takes BEGIN:END"):
        main([*base, "--inference", "--rows", "7"])
    with pytest.raises(SystemExit, match="--inference needs a pair range that is not empty"):
        main([*base, "--inference", "--pairs", "3:3"])
    with pytest.raises(SystemExit, match="family_alpha must be in"):
        main([("head2head.family_alpha=1.5" if a == "head2head.family_alpha=0.05" else a) for a in base] + ["--inference"])
    assert not (tmp_path / "never").exists()
