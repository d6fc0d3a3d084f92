"""`farkle run --seat-analysis`: per player count the reference's seat batch counts, seat effects and population effects, after the
last one the standardized effects, the exposure mixture, the self-play and the mirrored-game diagnostics — against the host
statement over the oracle's games (the stub engine serves them from rows; on the MI355X the HIP engine plays them), with the
reference's file names and schemas, two gloo ranks, the refusals, and an unchanged artifact set without the flag."""
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
SEAT_FILES = {"seat_batch_counts.parquet", "seat_effects.parquet", "seat_population_effects.parquet", "seat_effects_standardized_across_k.parquet",
              "seat_exposure_mixture.parquet", "seat_selfplay_p1.parquet", "seat_mirrored_games.parquet"}


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import seat_analysis_engine_stub

        stub = seat_analysis_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out", extra: str = "") -> Path:
    """configs/fast_config.yaml with its results under tmp_path and a coarser screening resolution (fewer shuffles)."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 4")
    path = tmp_path / f"{name}.yaml"
    path.write_text(text + extra)
    return path


def _expected(cfg_path: Path, weights=None):
    """Every frame of the stage from ONE stub call per player count over the run's whole shuffle range."""
    import seat_analysis_engine_stub

    from farkle_ii_amd import runner
    from farkle_ii_amd import seat_analysis as sa
    from farkle_ii_amd.config import load_app_config
    from farkle_ii_amd.strategies import pack_strategies

    cfg = load_app_config(cfg_path, seed_list_len=1)
    strategies, _ = runner._resolve_strategies(cfg, None)
    table = pack_strategies(strategies)
    ids = np.asarray([int(s.strategy_id) for s in strategies], dtype=np.int32)
    stub = seat_analysis_engine_stub.Engine(0)
    out = {"counts": {}, "by_k": {}, "population": {}}
    for k in KS:
        meta = pickle.loads((cfg.n_dir(k) / f"{k}p_checkpoint.pkl").read_bytes())["meta"]
        res = stub.tournament_seat_counts(table, k, cfg.sim.seed, 0, meta["num_shuffles"], shuffles_per_batch=meta["shuffles_per_batch"],
                                          strategy_ids=ids, want_mirrored=k == 2)
        counts = sa.SeatCounts.from_engine(res, k)
        out["counts"][k] = sa.batch_counts_table(counts, ids, cfg.sim.seed)
        out["by_k"][k], out["population"][k] = sa.within_k_frames(counts, ids, cfg.sim.seed)
        if k == 2:
            out["mirrored"] = sa.mirrored_frame(sa.MirroredPairs.from_engine(res, ids), cfg.sim.seed)
    w = sa.declared_weights(KS) if weights is None else sa.declared_weights(KS, "declared-mapping", weights)
    out["standardized"], out["mixture"] = sa.standardized_frames(out["by_k"], out["population"], KS, w)
    out["selfplay"] = sa.selfplay_frame(out["by_k"])
    return cfg, out


def _outputs(cfg):
    import pyarrow.parquet as pq

    return {"counts": {k: pq.read_table(cfg.seat_batch_counts_path(k)) for k in KS},
            "by_k": {k: pq.read_table(cfg.seat_effects_by_k_path(k)) for k in KS},
            "population": {k: pq.read_table(cfg.seat_population_by_k_path(k)) for k in KS},
            "standardized": pq.read_table(cfg.seat_standardized_across_k_path()), "mixture": pq.read_table(cfg.seat_exposure_mixture_diagnostic_path()),
            "selfplay": pq.read_table(cfg.seat_selfplay_diagnostic_path()), "mirrored": pq.read_table(cfg.seat_mirrored_diagnostic_path())}


def _same(got: dict, want: dict) -> None:
    for name, value in want.items():
        if isinstance(value, dict):
            for k in value:
                assert got[name][k].equals(value[k]), (name, k)
        else:
            assert got[name].equals(value), name


def _files(root: Path) -> set:
    return {str(p.relative_to(root)) for p in root.rglob("*") if p.is_file()}


def test_farkle_run_seat_analysis_writes_every_file(engine, tmp_path, monkeypatch):
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)  # several launch groups per player count
    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--seat-analysis"])
    cfg, want = _expected(cfg_path)
    got = _outputs(cfg)
    _same(got, want)
    # the reference's file names under the results root, and its schemas
    stage = cfg.results_root / cfg.io.analysis_subdir / "03_metrics"
    assert cfg.seat_batch_counts_path(4) == stage / "by_k" / "4p" / "seat_batch_counts.parquet"
    assert cfg.seat_standardized_across_k_path() == stage / "across_k" / "seat_effects_standardized_across_k.parquet"
    assert cfg.seat_mirrored_diagnostic_path() == stage / "diagnostics" / "seat_mirrored_games.parquet"
    assert [(f.name, str(f.type)) for f in got["counts"][2].schema] == [
        ("root_seed", "int64"), ("k", "int16"), ("deterministic_batch_id", "int32"), ("strategy", "int32"), ("seat", "int16"),
        ("raw_wins", "int64"), ("raw_exposures", "int64"), ("raw_completed_exposures", "int64"), ("raw_safety_limit_exposures", "int64")]
    assert got["by_k"][5].schema.names[-7:] == ["chance_baseline", "win_rate", "win_rate_per_attempt", "win_rate_given_completion",
                                                "safety_limit_exposure_rate", "raw_losses", "seat_effect"]
    assert got["standardized"].schema.names == ["root_seed", "effect_scope", "strategy", "seat", "common_k_support", "standardized_seat_effect"]
    assert got["standardized"].column("common_k_support").to_pylist()[0] == list(KS)
    assert set(got["standardized"].column("seat").to_pylist()) == {1, 2}  # the seats every player count has
    assert got["selfplay"].num_rows == 0  # unique strategy IDs and no one-player count
    assert got["mirrored"].schema.names[2:5] == ["strategy_a", "strategy_b", "paired_mirrored_games"] and got["mirrored"].num_rows > 0
    assert len(set(got["counts"][2].column("deterministic_batch_id").to_pylist())) >= 2
    # a complete run asked for seat counts it does not have is refused; --force replays it
    cfg.seat_batch_counts_path(4).unlink()
    with pytest.raises(ValueError, match="--force"):
        main(["--config", str(cfg_path), "run", "--seat-analysis"])
    main(["--config", str(cfg_path), "run", "--seat-analysis", "--force"])
    _same(_outputs(cfg), want)


def test_without_the_flag_the_artifact_set_is_unchanged(tmp_path):
    import seat_analysis_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    eng_mod.set_engine(seat_analysis_engine_stub.Engine(0))
    try:
        plain, seat = _config(tmp_path, name="plain"), _config(tmp_path, name="seat")
        main(["--config", str(plain), "run"])
        main(["--config", str(seat), "run", "--seat-analysis"])
        a = _files(load_app_config(plain, seed_list_len=1).results_root)
        b = _files(load_app_config(seat, seed_list_len=1).results_root)
        assert not any(Path(f).name in SEAT_FILES for f in a)
        assert a <= b and {Path(f).name for f in b - a} == SEAT_FILES and len(b - a) == 3 * len(KS) + 4
        # a run already complete without the counts: they need every game of it
        with pytest.raises(ValueError, match="--force"):
            main(["--config", str(plain), "run", "--seat-analysis"])
    finally:
        eng_mod.set_engine(None)


def test_settings_and_refusals(tmp_path):
    import seat_analysis_engine_stub

    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    eng_mod.set_engine(seat_analysis_engine_stub.Engine(0))
    try:
        declared = "k_aggregation:\n  method: declared-mapping\n  k_weights: {2: 0.5, 4: 0.3, 5: 0.2}\n"
        cfg_path = _config(tmp_path, extra=declared)
        main(["--config", str(cfg_path), "run", "--seat-analysis"])
        cfg, want = _expected(cfg_path, {2: 0.5, 4: 0.3, 5: 0.2})
        _same(_outputs(cfg), want)
        missing = _config(tmp_path, name="missing", extra="k_aggregation:\n  method: declared-mapping\n  k_weights: {2: 0.5, 4: 0.5}\n")
        with pytest.raises(ValueError, match="must cover every configured k"):
            main(["--config", str(missing), "run", "--seat-analysis"])
        for extra in (["--row-dir", str(tmp_path / "rows")], ["--rng-lag-sums"], ["--game-stats"]):
            with pytest.raises(ValueError, match="without rows"):
                main(["--config", str(_config(tmp_path, name="mixed")), "run", "--seat-analysis", "--force", *extra])
        # a checkpoint that already owns batches cannot be resumed with the flag: the counts span the whole run
        part = load_app_config(_config(tmp_path, name="part"), seed_list_len=1)
        runner.run_single_n(part, 2)
        (part.n_dir(2) / "simulation.done.json").unlink()  # (as if interrupted after its last checkpoint)
        part.sim.seat_analysis = True
        with pytest.raises(ValueError, match="already owns batches"):
            runner.run_single_n(part, 2)
    finally:
        eng_mod.set_engine(None)


def _run_rank(rank: int, world: int, port: int, cfg_path: str) -> None:
    for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import seat_analysis_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng_mod.set_engine(seat_analysis_engine_stub.Engine(0))
    runner.MAX_GAMES_PER_LAUNCH = 400  # several launch groups, each cut over the two ranks
    cfg = load_app_config(Path(cfg_path), seed_list_len=1)
    cfg.sim.seat_analysis = True
    runner.run_multi(cfg)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path, monkeypatch):
    import torch.multiprocessing as mp

    import seat_analysis_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    one = _config(tmp_path, name="one")
    two = _config(tmp_path, name="two")
    eng_mod.set_engine(seat_analysis_engine_stub.Engine(0))
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    try:
        main(["--config", str(one), "run", "--seat-analysis"])
    finally:
        eng_mod.set_engine(None)
    mp.spawn(_run_rank, args=(2, 41500 + os.getpid() % 2000, str(two)), nprocs=2, join=True)
    _same(_outputs(load_app_config(two, seed_list_len=1)), _outputs(load_app_config(one, seed_list_len=1)))
