"""`farkle run --roll-census`: the five kinds of file — the reference's two exact frames, the observed distribution, the fit and the
per-player-count strategy turn tables — against the host statement over the oracle's roll events (the stub engine serves the census
from tests/trace_oracle.py; on the MI355X the HIP engine counts on the device), with every other artifact of the run byte-equal to a
run without the flag; and the two census entry points in the built library."""
from __future__ import annotations

import hashlib
import re
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
SHUFFLES = 2


@pytest.fixture(params=["oracle-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    if request.param == "hip":
        eng_mod.set_engine(None)
        yield eng_mod.get_engine()
    else:
        import census_engine_stub

        stub = census_engine_stub.Engine(0)
        eng_mod.set_engine(stub)
        yield stub
    eng_mod.set_engine(None)


def _config(tmp_path: Path, name: str = "out") -> Path:
    """configs/fast_config.yaml with its results under tmp_path and a coarser screening resolution (fewer shuffles)."""
    text = (ROOT / "configs" / "fast_config.yaml").read_text()
    text = text.replace('results_dir_prefix: "results_fast_gpu"', f'results_dir_prefix: "{tmp_path / name}"')
    text = text.replace("resolution_delta: 0.03", "resolution_delta: 0.2").replace("target_batches: 100", "target_batches: 4")
    path = tmp_path / f"{name}.yaml"
    path.write_text(text)
    return path


def _snapshot(root: Path) -> dict:
    return {str(f.relative_to(root)): hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(root.rglob("*")) if f.is_file()}


def test_farkle_run_roll_census_writes_the_five_kinds_of_file(engine, tmp_path):
    import census_engine_stub
    import golden_util as gu
    import pyarrow as pa
    import pyarrow.parquet as pq

    from farkle_ii_amd import roll_census as rc
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config
    from farkle_ii_amd.strategies import pack_strategies

    cfg_path = _config(tmp_path)
    main(["--config", str(cfg_path), "run", "--roll-census", str(SHUFFLES)])
    cfg = load_app_config(cfg_path, seed_list_len=1)
    with_flag = _snapshot(cfg.results_root)
    census_files = [cfg.exact_roll_distribution_path(), cfg.exact_roll_summary_path(), cfg.observed_roll_distribution_path(), cfg.roll_fit_path(),
                    *[cfg.strategy_turns_path(k) for k in KS]]
    assert all(p.exists() for p in census_files)
    assert cfg.exact_roll_distribution_path().parent.name == "diagnostics" and cfg.strategy_turns_path(4).name == "4p_strategy_turns.parquet"

    # the exact frames: the reference's, bit for bit (tests/golden/roll_enumeration.json)
    golden = gu.load("roll_enumeration.json")
    for name, path in (("distribution", cfg.exact_roll_distribution_path()), ("summary", cfg.exact_roll_summary_path())):
        frame = pq.read_table(path).to_pandas()
        want = golden[name]
        assert list(frame.columns) == want["columns"] and [str(t) for t in frame.dtypes] == want["dtypes"]
        rows = [[v.hex() if isinstance(v, float) else (v.item() if hasattr(v, "item") else v) for v in row]
                for row in frame.itertuples(index=False, name=None)]
        assert rows == want["rows"], name

    # the observed frames: the host statement over the oracle's events of the same games
    strategies, _ = runner._resolve_strategies(cfg, None)
    table = pack_strategies(strategies)
    ids = [int(s.strategy_id) for s in strategies]
    stub = census_engine_stub.Engine(0)
    censuses = {k: rc.RollCensus.from_engine(stub.tournament_census(table, k, cfg.sim.seed, 0, SHUFFLES)) for k in KS}
    as_table = lambda frame: pa.Table.from_pandas(frame, preserve_index=False)  # noqa: E731
    observed = pq.read_table(cfg.observed_roll_distribution_path())
    assert observed.equals(as_table(rc.observed_table(censuses)))
    assert observed.num_rows == 127 * (1 + len(KS)) and sorted(set(observed.column("n_players").to_pylist())) == [0, *KS]
    merged = observed.to_pandas()
    per_k_total = int(merged.loc[merged["n_players"] != 0, "observed_count"].sum())
    assert int(merged.loc[merged["n_players"] == 0, "observed_count"].sum()) == per_k_total == sum(int(c.roll_cells.sum()) for c in censuses.values())
    assert pq.read_table(cfg.roll_fit_path()).equals(as_table(rc.fit_table(censuses)))
    for k in KS:
        turns = pq.read_table(cfg.strategy_turns_path(k))
        assert turns.equals(as_table(rc.strategy_turn_table(censuses[k], ids))), k
        assert turns.column("strategy").to_pylist() == ids and min(turns.column("turns").to_pylist()) > 0

    # every other artifact: byte for byte what the run writes without the flag
    shutil.rmtree(cfg.results_root)
    main(["--config", str(cfg_path), "run"])
    without = _snapshot(cfg.results_root)
    added = {str(p.relative_to(cfg.results_root)) for p in census_files}
    assert set(with_flag) - set(without) == added and set(without) <= set(with_flag)
    assert {name: with_flag[name] for name in without} == without


def test_roll_census_default_is_one_deterministic_batch_and_rank_zero_only(tmp_path, monkeypatch):
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import build_parser
    from farkle_ii_amd.config import load_app_config

    calls = []

    class Recorder:
        def tournament_census(self, table, k, root_seed, shuffle_begin, shuffle_end, **kw):
            from farkle_ii_amd.backend import _census_tables

            calls.append((k, shuffle_begin, shuffle_end, kw["shuffles_per_batch"]))
            return _census_tables(len(table), kw["turn_bins"])[0]

    args = build_parser().parse_args(["run", "--roll-census"])
    assert args.roll_census == 0 and build_parser().parse_args(["run"]).roll_census is None
    assert build_parser().parse_args(["run", "--roll-census", "7"]).roll_census == 7
    cfg = load_app_config(_config(tmp_path), seed_list_len=1)
    eng_mod.set_engine(Recorder())
    try:
        out = runner.run_roll_census(cfg, None)
        assert sorted(out) == list(KS) and [c[0] for c in calls] == list(KS)
        for k, lo, hi, spb in calls:
            plan = runner._plan_workload_from_config(cfg, 80, k)
            assert (lo, hi, spb) == (0, plan.shuffles_per_batch, plan.shuffles_per_batch) and hi <= plan.required_shuffles
        with pytest.raises(ValueError, match="positive"):
            runner.run_roll_census(cfg, -1)
        calls.clear()
        monkeypatch.setenv("RANK", "1")
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setattr(runner, "_rank_world", lambda: (1, 2))
        assert runner.run_roll_census(cfg, None) == {} and not calls
    finally:
        eng_mod.set_engine(None)


def test_library_exports_the_two_census_entry_points():
    from farkle_ii_amd import backend

    backend.build_library()
    lib = backend.load_library()
    header = (ROOT / "include" / "farkle_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|void|size_t|const char \*)\s*\*?(fk_\w+)\(", header, flags=re.M))
    for name in ("fk_census_games", "fk_tournament_run_census"):
        assert name in declared and name in backend.signatures() and hasattr(lib, name), name
    body = re.search(r"typedef struct \{([^}]*)\} fk_census;", header).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [name for name, _ in backend._Census._fields_]
    assert np.dtype(np.int64).itemsize == 8 and backend.CENSUS_ROLL_SHAPE == (6, 61, 7)
