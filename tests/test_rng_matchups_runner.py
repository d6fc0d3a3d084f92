"""`farkle run --rng-matchup-lags`: per player count the top-cap matchup groups, after the last one the root's matchup rows and
group-selection report — against the host statement of the rule over the oracle's games (the stub engine serves the records from
rows; on the MI355X the HIP engine plays and reduces), several launch groups and two gloo ranks included, and the refusals."""
from __future__ import annotations

import json
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

LAGS = (1, 2)


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import matchup_engine_stub

        stub = matchup_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, cap: int | None = 5, max_players: int = 12, name: str = "out") -> Path:
    path = tmp_path / f"{name}.yaml"
    path.write_text(f"""
io:
  results_dir_prefix: "{tmp_path / name}"
sim:
  n_players_list: [2, 4]
  seed_list: [7]
  expanded_metrics: true
  row_dir: null
  metric_chunk_dir: null
  score_thresholds: [300, 500]
  dice_thresholds: [1, 2]
  smart_five_opts: [true]
  smart_one_opts: [true, false]
  consider_score_opts: [true]
  consider_dice_opts: [true]
  auto_hot_dice_opts: [true]
  run_up_score_opts: [false]
screening:
  resolution_delta: 0.3
batching:
  target_batches: 4
  min_shuffles_per_batch: 2
analysis:
  rng_diagnostic_lags: [{", ".join(str(v) for v in LAGS)}]
  rng_diagnostic_partitions: 8
{f"  rng_max_matchup_groups: {cap}" if cap is not None else ""}
combine:
  max_players: {max_players}
""")
    return path


def _expected(cfg_path: Path):
    """The host statement over the oracle's games of every player count of the run: rows and report."""
    import matchup_engine_stub

    from farkle_ii_amd import rng_matchups as rm
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config
    from farkle_ii_amd.strategies import pack_strategies

    cfg = load_app_config(cfg_path, seed_list_len=1)
    strategies, _ = runner._resolve_strategies(cfg, None)
    table = pack_strategies(strategies)
    ids = np.asarray([int(s.strategy_id) for s in strategies], dtype=np.int32)
    cap = rm.effective_cap(cfg.rng_max_matchup_groups())
    stub = matchup_engine_stub.Engine(0)
    groups, fams = [], []
    for k in (2, 4):
        n_sh = pickle.loads((cfg.n_dir(k) / f"{k}p_checkpoint.pkl").read_bytes())["meta"]["num_shuffles"]
        rec = stub.tournament_matchups(table, k, 7, 0, n_sh, LAGS, ids, 12)["matchups"]
        groups.append(rm.MatchupGroups.from_reduce(rm.host_reduce(rec, k, LAGS, cap), ids, 12, cap))
        fams.append(rm.StrategyFamily(k, len(ids), n_sh))
    return cfg, rm.select(groups, fams, LAGS, cap, 8)


def _outputs(cfg):
    import pyarrow.parquet as pq

    return (pq.read_table(cfg.rng_matchup_stats_path()), json.loads(cfg.rng_group_selection_path().read_text()),
            [pq.read_table(cfg.rng_matchup_groups_path(k)) for k in (2, 4)])


def test_farkle_run_rng_matchup_lags_equals_the_host_statement(engine, tmp_path, monkeypatch):
    from farkle_ii_amd import rng_matchups as rm
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 40)  # several launch groups per player count
    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--rng-matchup-lags"])
    cfg, (rows, report) = _expected(cfg_path)
    stats, got_report, per_k = _outputs(cfg)
    assert got_report == json.loads(json.dumps(report))
    assert stats.equals(rm.stats_table(rows)) and stats.num_rows == len(LAGS) * report["selected_matchup_groups"]
    assert report["completeness_status"] == "blocked_by_cap" and report["selected_matchup_groups"] == 5
    assert set(stats.column("summary_level").to_pylist()) == {"matchup"}
    assert [t.num_rows for t in per_k] == [min(5, json.loads(t.schema.metadata[b"farkle_rng_matchup_groups"])["eligible_groups"]) for t in per_k]
    for k in (2, 4):  # the strategy family is written by the same pass; the per-k groups stay out of the authenticated outputs
        assert cfg.rng_lag_stats_path(k).exists() and cfg.rng_lag_sums_path(k).exists()
    done = json.loads((cfg.n_dir(2) / "simulation.done.json").read_text())
    assert any(p.endswith("2p_rng_matchup_groups.parquet") for p in done["outputs"])
    # a complete run asked for matchup files it does not have is refused; --force replays it
    main(["--config", str(cfg_path), "run", "--rng-matchup-lags"])  # (it has them: nothing to do)
    cfg.rng_matchup_groups_path(4).unlink()
    with pytest.raises(ValueError, match="--force"):
        main(["--config", str(cfg_path), "run", "--rng-matchup-lags"])
    main(["--config", str(cfg_path), "run", "--rng-matchup-lags", "--force"])
    assert _outputs(cfg)[0].equals(stats)


def test_uncapped_run_and_refusals(engine, tmp_path, monkeypatch):
    from farkle_ii_amd import rng_matchups as rm
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path, cap=None)
    text = cfg_path.read_text()
    main(["--config", str(cfg_path), "run", "--rng-matchup-lags"])
    cfg, (rows, report) = _expected(cfg_path)
    stats, got_report, _ = _outputs(cfg)
    assert got_report == json.loads(json.dumps(report)) and report["completeness_status"] == "planned_complete"
    assert stats.equals(rm.stats_table(rows))
    # combine.max_players must seat every player count; analysis settings are validated as the reference validates them
    for bad, match in (("max_players: 12", "max_players: 3"), ("rng_diagnostic_partitions: 8", "rng_diagnostic_partitions: 0")):
        cfg_path.write_text(text.replace(*(bad, match)))
        with pytest.raises(ValueError):
            main(["--config", str(cfg_path), "run", "--rng-matchup-lags", "--force"])
    cfg_path.write_text(text + "\n")
    with pytest.raises(ValueError, match="without rows"):
        main(["--config", str(cfg_path), "run", "--rng-matchup-lags", "--force", "--row-dir", str(tmp_path / "rows")])


def _run_rank(rank: int, world: int, port: int, cfg_path: str) -> None:
    for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import matchup_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng_mod.set_engine(matchup_engine_stub.Engine(0))
    runner.MAX_GAMES_PER_LAUNCH = 40  # several launch groups, each cut over the two ranks
    cfg = load_app_config(Path(cfg_path), seed_list_len=1)
    cfg.sim.rng_lag_sums = cfg.sim.rng_matchup_lags = True
    runner.run_multi(cfg)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path, monkeypatch):
    import torch.multiprocessing as mp

    import matchup_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    one = _config(tmp_path, name="one")
    two = _config(tmp_path, name="two")
    eng_mod.set_engine(matchup_engine_stub.Engine(0))
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 40)
    try:
        main(["--config", str(one), "run", "--rng-matchup-lags"])
    finally:
        eng_mod.set_engine(None)
    mp.spawn(_run_rank, args=(2, 37500 + os.getpid() % 2000, str(two)), nprocs=2, join=True)
    a = _outputs(load_app_config(one, seed_list_len=1))
    b = _outputs(load_app_config(two, seed_list_len=1))
    assert a[0].equals(b[0]) and a[1] == b[1] and all(x.equals(y) for x, y in zip(a[2], b[2]))
