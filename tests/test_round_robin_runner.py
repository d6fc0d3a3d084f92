"""`farkle round-robin` on the oracle stub engine (CPU) and on the HIP engine (MI355X): the files it writes equal the host module
(farkle_ii_amd/round_robin.py) called directly on the engine's states, and the command refuses what it must, naming the cause."""
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
BLOCK_GAMES, MULTIPLIER, MAX_ATTEMPTS = 12, 1.5, 18
PICK = (5, 0, 33, 79, 12, 48)  # positions in the grid, in file order (the command sorts by id)


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import round_robin_engine_stub

        stub = round_robin_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path) -> Path:
    """configs/fast_config.yaml (an 80-strategy grid) with its results under tmp_path."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / "out"}"')
    path = tmp_path / "cfg.yaml"
    path.write_text(text)
    return path


def _grid(cfg_path: Path):
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    cfg = load_app_config(cfg_path, seed_list_len=None)
    strategies, _ = runner._resolve_strategies(cfg, None)
    return cfg, sorted(strategies, key=lambda s: int(s.strategy_id))


def _base(cfg_path: Path) -> list[str]:
    return ["--config", str(cfg_path), "--set", f"sim.seed_list={ROOTS}", "--set", f"head2head.max_attempt_multiplier={MULTIPLIER}", "round-robin",
            "--block-games", str(BLOCK_GAMES)]


def test_round_robin_command_writes_what_the_host_module_states(engine, tmp_path):
    import pandas as pd

    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.strategies import pack_strategies

    cfg_path = _config(tmp_path)
    cfg, grid = _grid(cfg_path)
    assert len(grid) == 80
    chosen = sorted((grid[p] for p in PICK), key=lambda s: int(s.strategy_id))
    ids = [int(s.strategy_id) for s in chosen]
    ids_file = tmp_path / "family.txt"
    ids_file.write_text("".join(f"{int(grid[p].strategy_id)}\n" for p in PICK))
    out = tmp_path / "rr"
    main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--blocks", "--out", str(out)])
    assert sorted(f.name for f in out.iterdir()) == ["round_robin.json", "round_robin_blocks.parquet", "round_robin_pairs.parquet",
                                                     "round_robin_strategies.parquet"]
    # the same engine, called directly, and the host module on its states
    table = pack_strategies(chosen)
    summary = np.zeros((6, 8), dtype=np.int64)
    states = [engine.h2h_round_robin(table, root, BLOCK_GAMES, MAX_ATTEMPTS, summary=summary)[0] for root in ROOTS]
    want = {"blocks": rr.blocks_frame(ids, ROOTS, states, BLOCK_GAMES, MAX_ATTEMPTS), "pairs": rr.pairs_frame(ids, ROOTS, states, BLOCK_GAMES),
            "strategies": rr.strategies_frame(ids, summary)}
    for name, frame in want.items():
        got = pd.read_parquet(out / f"round_robin_{name}.parquet")
        assert list(got.columns) == list(frame.columns), name
        pd.testing.assert_frame_equal(got, frame, check_dtype=False, check_exact=True)
    assert len(want["blocks"]) == 15 * 2 * 2 and want["strategies"]["pairs"].tolist() == [5 * 2] * 6  # five opponents, two roots
    report = json.loads((out / "round_robin.json").read_text())
    attempted = int(sum(int(st[:, :, 0].sum()) for st in states))
    assert report["strategies"] == 6 and report["roots"] == ROOTS and report["block_games"] == BLOCK_GAMES
    assert report["max_attempts"] == MAX_ATTEMPTS and report["max_attempt_multiplier"] == MULTIPLIER
    assert (report["pair_begin"], report["pair_end"], report["pairs_total"], report["blocks"]) == (0, 15, 15, 60)
    assert report["games_attempted"] == attempted >= 60 * BLOCK_GAMES and report["elapsed_seconds"] >= 0
    assert report["games_completed"] == int(sum(int(st[:, :, 1].sum()) for st in states))

    # a pair range, without --blocks, into the default directory; then the existing directory is refused, and --force replaces it
    main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--pairs", "4:11"])
    default_dir = cfg.results_root / "h2h_round_robin"  # (the results root carries the first root of sim.seed_list: 42 in the file too)
    assert sorted(f.name for f in default_dir.iterdir()) == ["round_robin.json", "round_robin_pairs.parquet", "round_robin_strategies.parquet"]
    part = pd.read_parquet(default_dir / "round_robin_pairs.parquet")
    pd.testing.assert_frame_equal(part, want["pairs"].iloc[4:11].reset_index(drop=True), check_dtype=False, check_exact=True)
    part_summary = sum(rr.summary_from_states(6, st[4:11], BLOCK_GAMES, 4, 11) for st in states)
    assert np.array_equal(pd.read_parquet(default_dir / "round_robin_strategies.parquet")[list(rr.SUMMARY_COLS)].to_numpy(), part_summary)
    with pytest.raises(SystemExit, match="h2h_round_robin exists; pass --force"):
        main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--pairs", "4:11"])
    main([*_base(cfg_path), "--strategy-ids", str(ids_file), "--pairs", "0:2", "--force"])
    assert len(pd.read_parquet(default_dir / "round_robin_pairs.parquet")) == 2


def test_round_robin_command_refusals(engine, tmp_path, monkeypatch):
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    _, grid = _grid(cfg_path)
    known = [int(s.strategy_id) for s in grid]
    unknown = max(known) + 1

    def run(ids: list[int] | None, *extra: str, base: list[str] | None = None):
        args = list(base or _base(cfg_path))
        if ids is not None:
            ids_file = tmp_path / "ids.txt"
            ids_file.write_text("".join(f"{v}\n" for v in ids))
            args += ["--strategy-ids", str(ids_file)]
        main([*args, "--out", str(tmp_path / "never"), *extra])

    with pytest.raises(SystemExit, match="farkle round-robin: .*at least two strategies, got 1"):
        run(known[:1])
    with pytest.raises(SystemExit, match=rf"strategy ids not in the configuration's grid: \[{unknown}\]"):
        run([known[0], unknown, known[1]])
    with pytest.raises(SystemExit, match=rf"duplicate strategy ids in the id file: \[{known[3]}\]"):
        run([known[3], known[1], known[3]])
    with pytest.raises(SystemExit, match="--pairs takes BEGIN:END"):
        run(known[:4], "--pairs", "2")
    with pytest.raises(SystemExit, match=r"pair range \[2, 7\) is not inside the 6 pairs of 4 strategies"):
        run(known[:4], "--pairs", "2:7")
    with pytest.raises(SystemExit, match="head2head.max_attempt_multiplier must be finite and at least 1"):
        run(known[:4], base=["--config", str(cfg_path), "--set", "head2head.max_attempt_multiplier=0.5", "round-robin", "--block-games", "5"])
    with pytest.raises(SystemExit, match="--block-games must be at least 1"):
        run(known[:4], base=["--config", str(cfg_path), "round-robin", "--block-games", "0"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="runs on one rank, got a world of 2"):
        run(known[:4])
    monkeypatch.delenv("WORLD_SIZE")
    assert not (tmp_path / "never").exists()  # a refused command writes nothing
    run(known[:3], "--pairs", "1:3")          # ... and the engine still plays afterwards
    assert (tmp_path / "never" / "round_robin_pairs.parquet").exists()
