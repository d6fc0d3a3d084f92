"""`farkle round-robin --plan-power` on a CPU stub engine whose scan is the host statement (tests/power_plan_cases.py) and on the HIP
engine (MI355X): ``--plan-only`` writes the plan document and the power curve and plays nothing; ``--plan-power --inference`` writes
what ``--block-games <planned> --inference`` writes plus the three plan-derived columns; and what the flags refuse."""
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

import power_plan_cases as cases  # noqa: E402
from test_rr_inference_runner import _config  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "power_plan_vectors.json").read_text())
PICK = (3, 17, 40, 66)  # four strategies of the 80-strategy grid: the reference plans 43 games per block for them at delta 0.2 on one root
SETS = ("sim.seed_list=[42]", "head2head.practical_delta=0.2", "head2head.sensitivity_deltas=[0.2]", "head2head.min_candidate_completion_rate=0.5")
PLAN_FILES = ["h2h_power_curve.parquet", "h2h_power_plan.json"]
PLAN_COLUMNS = ["planned_target_power_conditional_on_completed_support", "planned_worst_scenario_power_conditional_on_completed_support",
                "power_support_status"]


def _stub_engine():
    import agreement_engine_stub

    class Engine(agreement_engine_stub.Engine, cases.HostStatementEngine):
        """The round robin of the oracle's blocks with the power scan's host statement; counts the calls that play."""

        def __init__(self, device=0):
            agreement_engine_stub.Engine.__init__(self, device)
            cases.HostStatementEngine.__init__(self)
            self.playing_calls = 0

        def h2h_round_robin(self, *a, **kw):
            self.playing_calls += 1
            return super().h2h_round_robin(*a, **kw)

        def h2h_round_robin_resident(self, *a, **kw):
            self.playing_calls += 1
            return super().h2h_round_robin_resident(*a, **kw)

    return Engine(0)


@pytest.fixture(params=["host-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    eng_mod.set_engine(None)
    stub = None
    if request.param == "host-stub":
        stub = _stub_engine()
        eng_mod.set_engine(stub)
    yield stub
    eng_mod.set_engine(None)


def _args(tmp_path: Path, *sets: str) -> list[str]:
    from farkle_ii_amd import runner
    from farkle_ii_amd.config import load_app_config

    cfg_path = _config(tmp_path)
    strategies, _ = runner._resolve_strategies(load_app_config(cfg_path, seed_list_len=None), None)
    grid = sorted(strategies, key=lambda s: int(s.strategy_id))
    ids_file = tmp_path / "family.txt"
    ids_file.write_text("".join(f"{int(grid[p].strategy_id)}\n" for p in PICK))
    return ["--config", str(cfg_path), *(a for s in (*SETS, *sets) for a in ("--set", s)), "round-robin", "--strategy-ids", str(ids_file)]


def test_plan_only_writes_the_plan_and_the_curve_and_plays_nothing(engine, tmp_path):
    import pandas as pd

    from farkle_ii_amd.cli import main

    out = tmp_path / "plan"
    main([*_args(tmp_path), "--plan-power", "--plan-only", "--out", str(out)])
    assert sorted(f.name for f in out.iterdir()) == PLAN_FILES  # no table of a played round robin, no round_robin.json
    if engine is not None:
        assert engine.playing_calls == 0 and engine.calls == 1
    doc = json.loads((out / "h2h_power_plan.json").read_text())
    want = GOLDEN["plans"]["four"]
    assert sorted(doc) == sorted(cases.DOCUMENT_KEYS)
    assert doc["n_completed_required_per_root_order_block"] == want["block_games"] == 43 and doc["root_seeds"] == [42]
    assert cases.hex_of(doc["worst_scenario_achieved_power"]) == want["worst_scenario_achieved_power"]
    assert cases.hex_of(doc["previous_equal_block_size_worst_power"]) == want["previous_equal_block_size_worst_power"]
    assert (doc["candidate_count"], doc["unordered_pair_count"], doc["alpha_per_pair"], doc["target_power"], doc["target_effect"]) == (4, 6, 0.02 / 6, 0.8, 0.2)
    assert [(r["reported_effect"], r["seat1_advantage"], r["games_per_order"]) for r in doc["power_validation"]] == [(0.2, s, 43) for s in cases.SCENARIOS]
    curve = pd.read_parquet(out / "h2h_power_curve.parquet")
    assert curve["block_games"].tolist() == list(range(1, 257)) and curve["games_per_order"].tolist() == list(range(1, 257))  # one window, one row per size
    assert list(curve.columns) == ["block_games", "games_per_order", "power_seat1_advantage_0", "power_seat1_advantage_0.03",
                                   "power_seat1_advantage_0.06", "worst_scenario_power"]
    worst = curve["worst_scenario_power"].to_numpy()
    assert np.array_equal(worst, curve.iloc[:, 2:5].min(axis=1).to_numpy())
    assert worst[42] >= 0.8 > worst[:42].max() and abs(worst[42] - doc["worst_scenario_achieved_power"]) < 1e-9
    with pytest.raises(SystemExit, match="exists; pass --force"):  # the directory is the command's, as for every round-robin run
        main([*_args(tmp_path), "--plan-power", "--plan-only", "--out", str(out)])


def test_plan_power_with_inference_equals_block_games_plus_three_columns(engine, tmp_path):
    import pandas as pd

    from farkle_ii_amd.cli import main

    planned, fixed = tmp_path / "planned", tmp_path / "fixed"
    main([*_args(tmp_path), "--plan-power", "--inference", "--out", str(planned)])
    main([*_args(tmp_path), "--block-games", "43", "--inference", "--out", str(fixed)])
    assert sorted(f.name for f in planned.iterdir()) == sorted([*(f.name for f in fixed.iterdir()), *PLAN_FILES])
    got, want = pd.read_parquet(planned / "round_robin_inference_pairs.parquet"), pd.read_parquet(fixed / "round_robin_inference_pairs.parquet")
    assert list(got.columns) == [*want.columns, *PLAN_COLUMNS] and not set(PLAN_COLUMNS) & set(want.columns)
    pd.testing.assert_frame_equal(got[list(want.columns)], want, check_exact=True)
    for name in ("round_robin_inference_strategies.parquet", "round_robin_strategies.parquet"):
        pd.testing.assert_frame_equal(pd.read_parquet(planned / name), pd.read_parquet(fixed / name), check_exact=True)
    doc = json.loads((planned / "h2h_power_plan.json").read_text())
    assert doc["n_completed_required_per_root_order_block"] == 43
    assert (got[PLAN_COLUMNS[0]] == 0.8).all() and (got[PLAN_COLUMNS[1]] == doc["worst_scenario_achieved_power"]).all()
    assert len(got) == 6 and (got["n_completed_required"] == 2 * 43).all()
    viable = got["pair_inferentially_viable"].to_numpy(dtype=bool)
    assert got["power_support_status"].tolist() == ["completed_support_achieved" if v else "unresolved_required_completed_support_not_achieved" for v in viable]
    assert viable.any()
    report, plain = json.loads((planned / "round_robin.json").read_text()), json.loads((fixed / "round_robin.json").read_text())
    assert report["block_games"] == plain["block_games"] == 43 and report["max_attempts"] == plain["max_attempts"]
    assert report["power_plan"]["n_completed_required_per_root_order_block"] == 43 and "power_plan" not in plain
    assert set(PLAN_FILES) <= set(report["files"]) and not set(PLAN_FILES) & set(plain["files"])
    assert {k: v for k, v in report.items() if k not in ("power_plan", "files", "elapsed_seconds")} == \
           {k: v for k, v in plain.items() if k not in ("files", "elapsed_seconds")}


def test_support_status_follows_viability():
    import pandas as pd

    from farkle_ii_amd import rr_inference as ri

    frame = pd.DataFrame({"pair_id": [0, 1, 2], "pair_inferentially_viable": [True, False, True]})
    got = ri.with_plan_columns(frame, 0.8, 0.81)
    assert list(got.columns) == ["pair_id", "pair_inferentially_viable", *PLAN_COLUMNS] and list(frame.columns) == ["pair_id", "pair_inferentially_viable"]
    assert got["power_support_status"].tolist() == ["completed_support_achieved", "unresolved_required_completed_support_not_achieved",
                                                    "completed_support_achieved"]
    assert got[PLAN_COLUMNS[0]].tolist() == [0.8] * 3 and got[PLAN_COLUMNS[1]].tolist() == [0.81] * 3


def test_flag_errors(tmp_path, capsys):
    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import AppConfig

    base = _args(tmp_path)
    for flags, message in ((["--block-games", "5", "--plan-power"], "not allowed with argument"), ([], "one of the arguments --block-games --plan-power is required"),
                           (["--block-games", "5", "--plan-only"], "--plan-only belongs to --plan-power")):
        with pytest.raises(SystemExit) as err:
            main([*base, *flags, "--out", str(tmp_path / "never")])
        assert err.value.code == 2 and message in capsys.readouterr().err
    assert not (tmp_path / "never").exists()
    for kw, message in ((dict(block_games=5, plan_power=True), "exactly one of"), (dict(block_games=None), "exactly one of"),
                        (dict(block_games=5, plan_only=True), "--plan-only belongs to --plan-power")):
        with pytest.raises(ValueError, match=message):
            rr.run_round_robin(AppConfig(), kw.pop("block_games"), **kw)
    with pytest.raises(SystemExit, match="single-root H2H is disabled by head2head.allow_single_root"):
        from farkle_ii_amd import engine as eng_mod

        eng_mod.set_engine(_stub_engine())
        try:
            main([*_args(tmp_path, "head2head.allow_single_root=false"), "--plan-power", "--plan-only", "--out", str(tmp_path / "never")])
        finally:
            eng_mod.set_engine(None)
