"""`farkle run --game-stats --rare-events`: after the last player count ``rare_events.parquet`` (game rows + summary rows),
``game_stats_rare_event_summary.parquet`` and, when asked, ``rare_events_details.parquet`` — against the host statement over the
oracle's games (the stub engine serves them from rows), with fixed and with quantile-resolved thresholds (a histograms-only pass,
then a replay that is checked against it), several launch groups, the capacity retry and the refusals."""
from __future__ import annotations

import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from test_game_stats_runner import KS, _config  # noqa: E402
from test_rare_events_cpu import encode  # noqa: E402


@pytest.fixture
def stub():
    import rare_events_engine_stub
    from farkle_ii_amd import engine as eng_mod

    engine = rare_events_engine_stub.Engine(0)
    eng_mod.set_engine(engine)
    yield engine
    eng_mod.set_engine(None)


def _expected(cfg_path: Path, thresholds=(500, 1000), rare_target=10_000, margin_quantile=None, target_rate=None):
    """The three tables from the host statement over the oracle's rows of the whole run, one call per player count."""
    import rare_events_engine_stub
    from farkle_ii_amd import rare_events as rev
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config
    from farkle_ii_amd.game_stats import rare_event_summary_table
    from farkle_ii_amd.strategies import pack_strategies

    cfg = load_app_config(cfg_path, seed_list_len=1)
    strategies, _ = runner._resolve_strategies(cfg, None)
    table = pack_strategies(strategies)
    ids = np.asarray([int(s.strategy_id) for s in strategies], dtype=np.int64)
    eng = rare_events_engine_stub.Engine(0)
    n_sh = {k: pickle.loads((cfg.n_dir(k) / f"{k}p_checkpoint.pkl").read_bytes())["meta"]["num_shuffles"] for k in KS}
    first = {k: eng.tournament_rare_events(table, k, cfg.sim.seed, 0, n_sh[k], rare_target_score=rare_target, want_events=False) for k in KS}
    summaries = {k: rev.RareEventSummary.from_engine(r, k) for k, r in first.items()}
    thr, target = rev.resolve_rare_event_thresholds(summaries, thresholds, rare_target, margin_quantile, target_rate)
    events = {}
    for k in KS:
        r = eng.tournament_rare_events(table, k, cfg.sim.seed, 0, n_sh[k], rare_target_score=target, thresholds=thr)["rare_events"]
        events[k] = (r["event_head"], r["event_seats"], len(table) // k, n_sh[k] * (len(table) // k))
    return {"cfg": cfg, "thresholds": thr, "target": target, "events": {k: len(e[0]) for k, e in events.items()},
            "rare_events": rev.rare_events_table(events, summaries, ids, thr, target),
            "details": rev.rare_event_details_table(events, ids, thr),
            "summary": rare_event_summary_table({k: s.under_target(target) for k, s in summaries.items()}, ids, thr)}


def _same(path: Path, want) -> None:
    import pyarrow.parquet as pq

    got = pq.read_table(path)
    assert got.schema.equals(want.schema) and encode(got) == encode(want), path.name  # (NaN margins: compared by bits)


def test_fixed_thresholds_write_the_files_in_one_pass(stub, tmp_path, monkeypatch):
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)  # several launch groups per player count: the lists concatenate
    analysis = "  game_stats_margin_thresholds: [100, 750]\n  rare_event_target_score: 2000\n  rare_event_write_details: true\n"
    cfg_path = _config(tmp_path, analysis=analysis)
    main(["--config", str(cfg_path), "run", "--game-stats", "--rare-events"])
    want = _expected(cfg_path, (100, 750), 2000)
    cfg = want["cfg"]
    assert all(0 < n for n in want["events"].values())
    _same(cfg.rare_events_path(), want["rare_events"])
    _same(cfg.rare_events_details_path(), want["details"])
    _same(cfg.game_stats_rare_summary_path(), want["summary"])
    assert all(c[5] for c in stub.calls) and {c[0] for c in stub.calls} == set(KS)  # one pass: every call collected events
    assert max(sum(1 for c in stub.calls if c[0] == k) for k in KS) >= 2  # ... over several ranges per player count
    ranges = [c[1:3] for c in stub.calls if c[0] == KS[0]]
    assert ranges == sorted(ranges) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


@pytest.mark.parametrize("analysis,kw", [
    ("  rare_event_margin_quantile: 0.05\n  rare_event_target_rate: 0.02\n", dict(margin_quantile=0.05, target_rate=0.02)),
    ("  rare_event_margin_quantile: 0.02\n  rare_event_target_score: 9000\n", dict(margin_quantile=0.02, rare_target=9000)),
    ("  rare_event_target_rate: 0.01\n  game_stats_margin_thresholds: [50]\n", dict(target_rate=0.01, thresholds=(50,))),
], ids=["both", "margin", "target"])
def test_quantile_mode_resolves_then_replays(stub, tmp_path, monkeypatch, analysis, kw):
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    cfg_path = _config(tmp_path, analysis=analysis)
    main(["--config", str(cfg_path), "run", "--game-stats", "--rare-events"])
    want = _expected(cfg_path, **kw)
    cfg = want["cfg"]
    if "margin_quantile" in kw:
        assert len(want["thresholds"]) == 1
    _same(cfg.rare_events_path(), want["rare_events"])
    _same(cfg.game_stats_rare_summary_path(), want["summary"])
    assert not cfg.rare_events_details_path().exists()  # not asked for
    first = [c for c in stub.calls if not c[5]]
    replay = [c for c in stub.calls if c[5]]
    assert first and replay and stub.calls == first + replay  # the histograms-only pass over EVERY player count comes first
    assert all(c[4] == () for c in first)
    assert all(c[3] == want["target"] and c[4] == tuple(want["thresholds"]) for c in replay)
    assert [c[:3] for c in first] == [c[:3] for c in replay]  # the same shuffle ranges


def test_the_replay_is_checked_against_the_first_pass(stub, tmp_path, monkeypatch):
    """A replay that plays other games than the first pass (here: a stub whose second pass shifts the root seed) is an error."""
    from farkle_ii_amd.cli import main

    plain = type(stub).tournament_rare_events

    def drifting(self, table, k, root_seed, *a, **kw):
        return plain(self, table, k, root_seed + (1 if kw.get("want_events", True) else 0), *a, **kw)

    monkeypatch.setattr(type(stub), "tournament_rare_events", drifting)
    cfg_path = _config(tmp_path, analysis="  rare_event_margin_quantile: 0.05\n")
    with pytest.raises(RuntimeError, match="replay"):
        main(["--config", str(cfg_path), "run", "--game-stats", "--rare-events"])


def test_refusals(stub, tmp_path):
    from farkle_ii_amd.cli import main

    with pytest.raises(ValueError, match="--game-stats"):
        main(["--config", str(_config(tmp_path)), "run", "--rare-events"])
    for analysis, match in (("  rare_event_margin_quantile: 1.0\n", "rare_event_margin_quantile must be between 0 and 1"),
                            ("  rare_event_target_rate: 0\n", "rare_event_target_rate must be between 0 and 1"),
                            ("  game_stats_margin_thresholds: [1, 2, 3, 4, 5, 6, 7, 8, 9]\n", "at most 8")):
        with pytest.raises(ValueError, match=match):
            main(["--config", str(_config(tmp_path, name="bad", analysis=analysis)), "run", "--game-stats", "--rare-events", "--force"])
    for extra in (["--row-dir", str(tmp_path / "rows")], ["--rng-lag-sums"]):
        with pytest.raises(ValueError, match="without rows"):
            main(["--config", str(_config(tmp_path, name="mixed")), "run", "--game-stats", "--rare-events", "--force", *extra])
    # without the new flag the quantile keys stay refused
    with pytest.raises(ValueError, match="fixed thresholds"):
        main(["--config", str(_config(tmp_path, name="q", analysis="  rare_event_target_rate: 0.1\n")), "run", "--game-stats"])
    # a sweep of which a player count is already complete cannot add its games
    done = _config(tmp_path, name="done")
    main(["--config", str(done), "run", "--game-stats"])
    with pytest.raises(ValueError, match="--force"):
        main(["--config", str(done), "run", "--game-stats", "--rare-events"])


def test_partial_checkpoint_is_refused(stub, tmp_path):
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    cfg = load_app_config(_config(tmp_path), seed_list_len=1)
    runner.run_single_n(cfg, 2)
    (cfg.n_dir(2) / "simulation.done.json").unlink()  # (as if interrupted after its last checkpoint)
    cfg.sim.game_stats = cfg.sim.rare_events = True
    with pytest.raises(ValueError, match="already owns batches"):
        runner.run_single_n(cfg, 2)


def test_capacity_retry_and_merged_ranges(stub):
    """A list that does not fit is replayed with the reported room; two ranges merged equal the one."""
    from tools.time_config import table_for

    from farkle_ii_amd import rare_events as rev
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    t = table_for(64)
    kw = dict(target_score=3000, rare_target_score=2000, thresholds=(100, 500))
    whole = stub.tournament_rare_events(t, 4, 9, 0, 20, **kw)
    n = whole["rare_events"]["events"]
    assert n > 2 and whole["attempts"] == 1
    with pytest.raises(FarkleHipError) as err:
        stub.tournament_rare_events(t, 4, 9, 0, 20, event_capacity=n - 1, retry=False, **kw)
    assert err.value.code == FK_ERR_ARG and err.value.events_needed == n
    again = stub.tournament_rare_events(t, 4, 9, 0, 20, event_capacity=n - 1, **kw)
    assert again["attempts"] == 2 and np.array_equal(again["rare_events"]["event_head"], whole["rare_events"]["event_head"])
    a, b = stub.tournament_rare_events(t, 4, 9, 0, 7, **kw), stub.tournament_rare_events(t, 4, 9, 7, 20, **kw)
    head, seats = rev.concat_events([(p["rare_events"]["event_head"], p["rare_events"]["event_seats"]) for p in (a, b)], [0, 7])
    assert np.array_equal(head, whole["rare_events"]["event_head"]) and np.array_equal(seats, whole["rare_events"]["event_seats"])
    merged = rev.RareEventSummary.from_engine(a, 4).merge(rev.RareEventSummary.from_engine(b, 4))
    one = rev.RareEventSummary.from_engine(whole, 4)
    assert np.array_equal(merged.game_second, one.game_second) and np.array_equal(merged.strategy_second, one.strategy_second)


def _run_rank(rank: int, world: int, port: int, cfg_path: str) -> None:
    import os

    for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import rare_events_engine_stub
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng_mod.set_engine(rare_events_engine_stub.Engine(0))
    runner.MAX_GAMES_PER_LAUNCH = 400  # several launch groups, each cut over the two ranks
    cfg = load_app_config(Path(cfg_path), seed_list_len=1)
    cfg.sim.game_stats = cfg.sim.rare_events = True
    runner.run_multi(cfg)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(stub, tmp_path, monkeypatch):
    """A batch is played whole by one rank: events concatenate in rank order, histograms add; the quantile replay runs on rank 0."""
    import os

    import pyarrow.parquet as pq
    import torch.multiprocessing as mp

    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    analysis = "  rare_event_margin_quantile: 0.05\n  rare_event_write_details: true\n"
    one, two = _config(tmp_path, name="one", analysis=analysis), _config(tmp_path, name="two", analysis=analysis)
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    main(["--config", str(one), "run", "--game-stats", "--rare-events"])
    mp.spawn(_run_rank, args=(2, 41500 + os.getpid() % 2000, str(two)), nprocs=2, join=True)
    a, b = load_app_config(one, seed_list_len=1), load_app_config(two, seed_list_len=1)
    for name in ("rare_events_path", "rare_events_details_path", "game_stats_rare_summary_path"):
        ta, tb = pq.read_table(getattr(a, name)()), pq.read_table(getattr(b, name)())
        assert ta.num_rows > 0 and ta.schema.equals(tb.schema) and encode(ta) == encode(tb), name


@pytest.mark.gpu
def test_hip_engine_quantile_mode_end_to_end(tmp_path, monkeypatch):
    """The same command on the MI355X: the HIP engine plays both passes; the files equal the host statement over the oracle's rows."""
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main

    eng_mod.set_engine(None)
    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    try:
        analysis = "  rare_event_margin_quantile: 0.05\n  rare_event_target_rate: 0.02\n  rare_event_write_details: true\n"
        cfg_path = _config(tmp_path, analysis=analysis)
        main(["--config", str(cfg_path), "run", "--game-stats", "--rare-events"])
        want = _expected(cfg_path, margin_quantile=0.05, target_rate=0.02)
        _same(want["cfg"].rare_events_path(), want["rare_events"])
        _same(want["cfg"].rare_events_details_path(), want["details"])
        _same(want["cfg"].game_stats_rare_summary_path(), want["summary"])
    finally:
        eng_mod.set_engine(None)
