"""`farkle run --game-stats`: per player count the reference's game-stats table and its exact histograms, after the last one the
root's rare-event summary — against the host statement over the oracle's games (the stub engine serves them from rows; on the
MI355X the HIP engine plays them), with the all-player batches on the same launches, two gloo ranks, and the refusals."""
from __future__ import annotations

import os
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

KS = (2, 4, 5)


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import game_stats_engine_stub

        stub = game_stats_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out", analysis: str = "") -> Path:
    """configs/fast_config.yaml with its results under tmp_path and a coarser screening resolution (fewer shuffles)."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 4")
    path = tmp_path / f"{name}.yaml"
    path.write_text(text + (f"analysis:\n{analysis}" if analysis else ""))
    return path


def _expected(cfg_path: Path, thresholds=(500, 1000), rare_target=10_000):
    import game_stats_engine_stub

    from farkle_ii_amd import game_stats as gs
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config
    from farkle_ii_amd.strategies import pack_strategies

    cfg = load_app_config(cfg_path, seed_list_len=1)
    strategies, _ = runner._resolve_strategies(cfg, None)
    table = pack_strategies(strategies)
    ids = np.asarray([int(s.strategy_id) for s in strategies], dtype=np.int64)
    stub = game_stats_engine_stub.Engine(0)
    per_k = {}
    for k in KS:
        n_sh = pickle.loads((cfg.n_dir(k) / f"{k}p_checkpoint.pkl").read_bytes())["meta"]["num_shuffles"]
        per_k[k] = gs.GameStatsSummary.from_engine(stub.tournament_game_stats(table, k, cfg.sim.seed, 0, n_sh, rare_target_score=rare_target), k)
    tables = {k: gs.game_stats_table(s, ids, k, thresholds) for k, s in per_k.items()}
    return cfg, ids, per_k, tables, gs.rare_event_summary_table(per_k, ids, thresholds)


def _outputs(cfg):
    import pyarrow.parquet as pq

    return ([pq.read_table(cfg.game_stats_path(k)) for k in KS], [pq.read_table(cfg.game_stats_sums_path(k)) for k in KS],
            pq.read_table(cfg.game_stats_rare_summary_path()))


def test_farkle_run_game_stats_writes_the_three_files(engine, tmp_path, monkeypatch):
    from farkle_ii_amd import game_stats as gs
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)  # several launch groups per player count
    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--game-stats", "--all-player-batches"])
    cfg, ids, per_k, tables, rare = _expected(cfg_path)
    got_tables, got_sums, got_rare = _outputs(cfg)
    cfg.sim.all_player_batch_dir = Path("all_player_batches")  # (the flag's default directory)
    for k, got, sums in zip(KS, got_tables, got_sums):
        assert got.equals(tables[k]), k
        back = gs.GameStatsSummary.from_sums_table(sums, ids, k)
        assert gs.game_stats_table(back, ids, k).equals(tables[k])
        assert (cfg.all_player_batch_dir(k) / "all_player_manifest.jsonl").exists()  # the all-player batches rode on the same launches
    assert rare is not None and got_rare.equals(rare)
    assert set(got_rare.column("n_players").to_pylist()) == set(KS)
    # a complete run asked for game statistics it does not have is refused; --force replays it
    cfg.game_stats_sums_path(4).unlink()
    with pytest.raises(ValueError, match="--force"):
        main(["--config", str(cfg_path), "run", "--game-stats"])
    main(["--config", str(cfg_path), "run", "--game-stats", "--force"])
    assert _outputs(cfg)[0][1].equals(tables[4])


def test_settings_and_refusals(tmp_path):
    import game_stats_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd.cli import main

    eng_mod.set_engine(game_stats_engine_stub.Engine(0))
    try:
        cfg_path = _config(tmp_path, analysis="  game_stats_margin_thresholds: [100, 750]\n  rare_event_target_score: 2000\n")
        main(["--config", str(cfg_path), "run", "--game-stats"])
        cfg, _, _, tables, rare = _expected(cfg_path, (100, 750), 2000)
        got_tables, _, got_rare = _outputs(cfg)
        assert all(got_tables[i].equals(tables[k]) for i, k in enumerate(KS)) and got_rare.equals(rare)
        assert "prob_margin_runner_up_le_750" in got_tables[0].schema.names and "margin_le_100" in got_rare.schema.names
        for analysis, match in (("  rare_event_margin_quantile: 0.01\n", "fixed thresholds"), ("  rare_event_target_rate: 0.1\n", "fixed thresholds"),
                                ("  game_stats_margin_thresholds: oops\n", "integers")):
            with pytest.raises(ValueError, match=match):
                main(["--config", str(_config(tmp_path, name="bad", analysis=analysis)), "run", "--game-stats", "--force"])
        for extra in (["--row-dir", str(tmp_path / "rows")], ["--rng-lag-sums"]):
            with pytest.raises(ValueError, match="without rows"):
                main(["--config", str(_config(tmp_path, name="mixed")), "run", "--game-stats", "--force", *extra])
        # a run already complete without the statistics: they need every game of it
        plain = _config(tmp_path, name="plain")
        main(["--config", str(plain), "run"])
        with pytest.raises(ValueError, match="--force"):
            main(["--config", str(plain), "run", "--game-stats"])
    finally:
        eng_mod.set_engine(None)


def test_partial_checkpoint_is_refused(tmp_path):
    """A checkpoint that already owns batches cannot be resumed with --game-stats: the histograms span the whole run."""
    import game_stats_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    eng_mod.set_engine(game_stats_engine_stub.Engine(0))
    try:
        cfg = load_app_config(_config(tmp_path), seed_list_len=1)
        runner.run_single_n(cfg, 2)
        (cfg.n_dir(2) / "simulation.done.json").unlink()  # (as if interrupted after its last checkpoint)
        cfg.sim.game_stats = True
        with pytest.raises(ValueError, match="already owns batches"):
            runner.run_single_n(cfg, 2)
    finally:
        eng_mod.set_engine(None)


def _run_rank(rank: int, world: int, port: int, cfg_path: str) -> None:
    for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import game_stats_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng_mod.set_engine(game_stats_engine_stub.Engine(0))
    runner.MAX_GAMES_PER_LAUNCH = 400  # several launch groups, each cut over the two ranks
    cfg = load_app_config(Path(cfg_path), seed_list_len=1)
    cfg.sim.game_stats = True
    runner.run_multi(cfg)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path, monkeypatch):
    import torch.multiprocessing as mp

    import game_stats_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    one = _config(tmp_path, name="one")
    two = _config(tmp_path, name="two")
    eng_mod.set_engine(game_stats_engine_stub.Engine(0))
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    try:
        main(["--config", str(one), "run", "--game-stats"])
    finally:
        eng_mod.set_engine(None)
    mp.spawn(_run_rank, args=(2, 39500 + os.getpid() % 2000, str(two)), nprocs=2, join=True)
    a = _outputs(load_app_config(one, seed_list_len=1))
    b = _outputs(load_app_config(two, seed_list_len=1))
    assert all(x.equals(y) for x, y in zip(a[0], b[0])) and all(x.equals(y) for x, y in zip(a[1], b[1])) and a[2].equals(b[2])
