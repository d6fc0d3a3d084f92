"""`farkle run --performance-bootstrap`: per player count the reference's batch matrix, after the last one the joint batch bootstrap's
two frames — against the host statement applied to the all-player batch table of the same run (the stub engine serves the bootstrap
with the host statement; on the MI355X the HIP engine computes it and must write the same files), the schemas, the refusals, two gloo
ranks."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

KS = (2, 4, 5)
SCREENING = "  bootstrap_replicates: 60\n  delta_across_k: 0.02\n  candidate_contribution_size: 7\n  controls: [3, 41, 3]\n"


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import performance_bootstrap_engine_stub

        stub = performance_bootstrap_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out", screening: str = SCREENING) -> Path:
    """configs/fast_config.yaml with its results under tmp_path, a coarser screening resolution (fewer shuffles), six batches and the
    bootstrap's settings."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 6")
    assert "interval_confidence: 0.95\n" in text
    text = text.replace("interval_confidence: 0.95\n", "interval_confidence: 0.95\n" + screening)
    path = tmp_path / f"{name}.yaml"
    path.write_text(text)
    return path


def _matrices_from_batch_tables(cfg) -> dict:
    """The reference's route to the matrices (``_write_batch_matrix``): the all-player batch table of the run."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from farkle_ii_amd import performance_bootstrap as pb

    out = {}
    for k in KS:
        d = cfg.all_player_batch_dir(k)
        t = pa.concat_tables([pq.read_table(p) for p in sorted(d.glob("all_player_batch_*.parquet"))])
        batches, strategies = np.unique(t.column("deterministic_batch_id").to_numpy()), np.unique(t.column("strategy").to_numpy())
        assert t.num_rows == len(batches) * len(strategies)  # rectangular
        pos = np.searchsorted(batches, t.column("deterministic_batch_id").to_numpy()) * len(strategies) + np.searchsorted(
            strategies, t.column("strategy").to_numpy())
        cells = {}
        for name in ("raw_wins", "raw_player_game_exposures", "raw_completed_player_game_exposures", "raw_safety_limit_player_game_exposures"):
            flat = np.zeros(len(pos), np.int64)
            flat[pos] = t.column(name).to_numpy()
            cells[name] = flat.reshape(len(batches), len(strategies))
        out[k] = pb.BatchMatrix(int(cfg.sim.seed), k, batches.astype(np.int32), strategies.astype(np.int32), cells["raw_wins"],
                                cells["raw_player_game_exposures"], cells["raw_completed_player_game_exposures"],
                                cells["raw_safety_limit_player_game_exposures"])
    return out


def _outputs(cfg):
    import pyarrow.parquet as pq

    return pq.read_table(cfg.performance_bootstrap_path()), pq.read_table(cfg.performance_control_contrasts_path())


def test_farkle_run_performance_bootstrap_writes_matrices_and_frames(engine, tmp_path, monkeypatch):
    import performance_bootstrap_engine_stub

    from farkle_ii_amd import performance_bootstrap as pb
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)  # several launch groups per player count
    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--performance-bootstrap", "--all-player-batches"])
    cfg = load_app_config(cfg_path, seed_list_len=1)
    cfg.sim.all_player_batch_dir = Path("all_player_batches")  # (the flag's default directory)
    matrices = _matrices_from_batch_tables(cfg)
    for k in KS:
        path = cfg.performance_batch_matrix_path(k)
        assert path == cfg.results_root / "analysis" / "03_metrics" / "by_k" / f"{k}p" / "performance_batch_matrix.npy"
        got = np.load(path)
        assert got.dtype == pb.BATCH_MATRIX_DTYPE and got.shape == (6, 80)
        assert got.tobytes() == matrices[k].to_reference_array().tobytes()
    want_boot, want_contrasts = pb.performance_bootstrap_tables(performance_bootstrap_engine_stub.Engine(0), matrices, KS, 60, 7, 0.02, [3, 41])
    boot, contrasts = _outputs(cfg)
    assert cfg.performance_bootstrap_path().parent == cfg.results_root / "analysis" / "03_metrics" / "across_k"
    assert boot.schema.equals(pb.bootstrap_schema()) and contrasts.schema.equals(pb.contrast_schema())
    assert boot.equals(want_boot) and contrasts.equals(want_contrasts)
    assert boot.num_rows == 80 and contrasts.num_rows == 160 and set(contrasts.column("control_strategy").to_pylist()) == {3, 41}
    assert boot.column("top_n_size").to_pylist() == [7] * 80 and boot.column("bootstrap_replicates").to_pylist() == [60] * 80
    assert sum(boot.column("top_n_inclusion_probability").to_pylist()) == pytest.approx(7.0)  # (a sanity reading, not the check)
    # a complete run asked for matrices it does not have is refused; --force replays it, without the all-player batches too
    cfg.performance_batch_matrix_path(4).unlink()
    with pytest.raises(ValueError, match="--force"):
        main(["--config", str(cfg_path), "run", "--performance-bootstrap"])
    main(["--config", str(cfg_path), "run", "--performance-bootstrap", "--force"])
    again = _outputs(cfg)
    assert again[0].equals(want_boot) and again[1].equals(want_contrasts)
    assert np.load(cfg.performance_batch_matrix_path(4)).tobytes() == matrices[4].to_reference_array().tobytes()


def test_refusals(tmp_path):
    import performance_bootstrap_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    eng_mod.set_engine(performance_bootstrap_engine_stub.Engine(0))
    try:
        for screening, match in ((SCREENING.replace("delta_across_k: 0.02", "delta_across_k: null"), "delta_across_k is required"),
                                 (SCREENING.replace("[3, 41, 3]", "[3, 4100]"), "controls lack complete k support: \\[4100\\]"),
                                 (SCREENING.replace("bootstrap_replicates: 60", "bootstrap_replicates: 0"), "bootstrap_replicates")):
            bad = _config(tmp_path, name="bad", screening=screening)
            with pytest.raises(ValueError, match=match):
                main(["--config", str(bad), "run", "--performance-bootstrap", "--force"])
            assert not load_app_config(bad, seed_list_len=1).n_dir(2).exists()  # refused before anything played
        for extra in (["--row-dir", str(tmp_path / "rows")], ["--rng-lag-sums"]):
            with pytest.raises(ValueError, match="without rows"):
                main(["--config", str(_config(tmp_path, name="mixed")), "run", "--performance-bootstrap", "--force", *extra])
        plain = _config(tmp_path, name="plain")  # a run already complete without the matrices: they need every batch of it
        main(["--config", str(plain), "run"])
        with pytest.raises(ValueError, match="--force"):
            main(["--config", str(plain), "run", "--performance-bootstrap"])
        # a checkpoint that already owns batches cannot be resumed: the batch statistics of the earlier launches are gone
        cfg = load_app_config(_config(tmp_path, name="partial"), seed_list_len=1)
        runner.run_single_n(cfg, 2)
        (cfg.n_dir(2) / "simulation.done.json").unlink()  # (as if interrupted after its last checkpoint)
        cfg.sim.performance_bootstrap = True
        with pytest.raises(ValueError, match="already owns batches"):
            runner.run_single_n(cfg, 2)
    finally:
        eng_mod.set_engine(None)


def test_one_player_count_and_game_stats_together(tmp_path):
    """A single player count goes the same way (the frames follow it), and --game-stats shares the statistics launch."""
    import game_stats_engine_stub
    import performance_bootstrap_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    class Both(performance_bootstrap_engine_stub.Engine, game_stats_engine_stub.Engine):
        pass

    eng_mod.set_engine(Both(0))
    try:
        path = _config(tmp_path)
        path.write_text(path.read_text().replace("n_players_list: [2, 4, 5]", "n_players_list: [4]"))
        main(["--config", str(path), "run", "--performance-bootstrap", "--game-stats"])
        cfg = load_app_config(path, seed_list_len=1)
        boot, contrasts = _outputs(cfg)
        assert boot.num_rows == 80 and contrasts.num_rows == 160 and cfg.game_stats_path(4).exists()
    finally:
        eng_mod.set_engine(None)


def _run_rank(rank: int, world: int, port: int, cfg_path: str) -> None:
    for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import performance_bootstrap_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng_mod.set_engine(performance_bootstrap_engine_stub.Engine(0))
    runner.MAX_GAMES_PER_LAUNCH = 400  # several launch groups, each cut over the two ranks
    cfg = load_app_config(Path(cfg_path), seed_list_len=1)
    cfg.sim.performance_bootstrap = True
    runner.run_multi(cfg)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path, monkeypatch):
    import torch.multiprocessing as mp

    import performance_bootstrap_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    one = _config(tmp_path, name="one")
    two = _config(tmp_path, name="two")
    eng_mod.set_engine(performance_bootstrap_engine_stub.Engine(0))
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    try:
        main(["--config", str(one), "run", "--performance-bootstrap"])
    finally:
        eng_mod.set_engine(None)
    mp.spawn(_run_rank, args=(2, 41500 + os.getpid() % 2000, str(two)), nprocs=2, join=True)
    c1, c2 = load_app_config(one, seed_list_len=1), load_app_config(two, seed_list_len=1)
    for k in KS:
        assert np.load(c1.performance_batch_matrix_path(k)).tobytes() == np.load(c2.performance_batch_matrix_path(k)).tobytes()
    a, b = _outputs(c1), _outputs(c2)
    assert a[0].equals(b[0]) and a[1].equals(b[1])
