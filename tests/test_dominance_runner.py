"""`farkle round-robin --inference --dominance` on the CPU stub engine (tests/dominance_engine_stub.py) and on the HIP engine (MI355X):
the four digest artifacts it writes equal the frames of the host statement (``farkle_ii_amd.dominance``) over the inference rows of
the same run; the edges are left out, and the report says so, when not every pair's row comes to the host; and what the option
refuses."""
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

from test_rr_inference_runner import KNOBS, _base, _config, _family  # noqa: E402  (the same family and settings)

DOMINANCE_FILES = ["cycle_groups.parquet", "dominance_edges.parquet", "dominance_fronts.parquet", "dominance_summary.json"]


@pytest.fixture(params=["host-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    eng_mod.set_engine(None)
    if request.param == "host-stub":
        import dominance_engine_stub

        eng_mod.set_engine(dominance_engine_stub.Engine(0))
    yield request.param
    eng_mod.set_engine(None)


def _assert_frames_equal(got, want):
    import dominance_cases as cases

    assert cases.frame_records(got)["rows"] == cases.frame_records(want)["rows"] and list(got.columns) == list(want.columns)


def test_dominance_command_writes_the_frames_of_the_host_statement(engine, tmp_path):
    import pandas as pd

    from farkle_ii_amd import dominance as dom
    from farkle_ii_amd import rr_inference as ri
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    scores = {str(s): 0.25 * (k % 3) for k, s in enumerate(ids)}
    scores_file = tmp_path / "scores.json"
    scores_file.write_text(json.dumps(scores))
    out = tmp_path / "rr"
    args = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--inference", "--dominance", "--out", str(out)]
    main([*args, "--screening-scores", str(scores_file)])
    assert sorted(f.name for f in out.iterdir()) == sorted(DOMINANCE_FILES + ["round_robin.json", "round_robin_inference_pairs.parquet",
                                                                             "round_robin_inference_strategies.parquet", "round_robin_strategies.parquet"])
    # the host statement over the rows this run wrote
    pairs = pd.read_parquet(out / "round_robin_inference_pairs.parquet")
    strategies = pd.read_parquet(out / "round_robin_inference_strategies.parquet")
    cls = np.array([ri.DECISION_CLASSES.index(c) for c in pairs["decision_class"]], dtype=np.uint8)
    low, high = pairs["simultaneous_d_low"].to_numpy(), pairs["simultaneous_d_high"].to_numpy()
    rate = pairs["balanced_a_win_rate_alias"].to_numpy()
    host = dom.graph(8, cls, low, high, rate, KNOBS["practical_delta"], rank=dom.rank_of_ids(ids))
    st = np.zeros((8, 12), dtype=np.int64)
    st[:, 7], st[:, 8] = strategies["games_attempted"], strategies["games_completed"]
    st[:, 10], st[:, 11] = strategies["operationally_viable"], strategies["inferentially_viable"]
    from farkle_ii_amd.backend import RR_PAIR_ROW_DTYPE

    rows = np.zeros(28, dtype=RR_PAIR_ROW_DTYPE)
    rows["pair_id"], rows["decision_class"], rows["d_ab"] = pairs["pair_id"], cls, pairs["d_ab"]
    rows["simultaneous_d_low"], rows["simultaneous_d_high"] = low, high
    rows["strategy_a"] = [ids.index(v) for v in pairs["strategy_a"]]
    rows["strategy_b"] = [ids.index(v) for v in pairs["strategy_b"]]
    _assert_frames_equal(pd.read_parquet(out / "dominance_edges.parquet"), dom.edges_frame(rows, ids, KNOBS["practical_delta"]))
    _assert_frames_equal(pd.read_parquet(out / "dominance_fronts.parquet"), dom.fronts_frame(host["nodes"], st, ids, {int(k): v for k, v in scores.items()}))
    _assert_frames_equal(pd.read_parquet(out / "cycle_groups.parquet"), dom.cycles_frame(host["nodes"], host["extremes"], host["adjacency"], ids))
    report = json.loads((out / "round_robin.json").read_text())
    counts = np.array([report["inference"]["class_counts"][name] for name in ri.DECISION_CLASSES])
    assert json.loads((out / "dominance_summary.json").read_text()) == dom.summary(host["nodes"], st, counts, ids)
    assert report["dominance"]["edges_written"] is True and set(DOMINANCE_FILES) <= set(report["files"])
    assert counts[:4].sum() > 0  # the family has directed pairs: the graphs are not empty
    # a slice of the rows: no edge table, and the report says so; no scores: the column is null
    main([*args, "--rows", "5:9", "--force"])
    report = json.loads((out / "round_robin.json").read_text())
    assert report["dominance"]["edges_written"] is False and "edges_omitted" in report["dominance"]
    assert "dominance_edges.parquet" not in report["files"]
    fronts = pd.read_parquet(out / "dominance_fronts.parquet")
    assert fronts["tournament_screening_score"].isna().all() and len(fronts) == 8


def test_dominance_option_refusals(tmp_path):
    """Refused while reading the command line and the configuration: no engine is asked for."""
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    _, ids_file = _family(cfg_path, tmp_path)
    base = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--out", str(tmp_path / "never")]
    with pytest.raises(SystemExit, match="--dominance belongs to --inference"):
        main([*base, "--dominance"])
    with pytest.raises(SystemExit, match=r"--dominance needs every pair of the table, --pairs plays \[4, 20\) of 28"):
        main([*base, "--inference", "--dominance", "--pairs", "4:20"])
    with pytest.raises(SystemExit, match="--screening-scores belongs to --dominance"):
        main([*base, "--inference", "--screening-scores", str(ids_file)])
    short = tmp_path / "short.json"
    short.write_text("{}")
    with pytest.raises(SystemExit, match="lacks the screening scores of strategies"):
        main([*base, "--inference", "--dominance", "--screening-scores", str(short)])
    assert not (tmp_path / "never").exists()
