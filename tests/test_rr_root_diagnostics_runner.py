"""`farkle round-robin --inference --root-diagnostics` on the CPU stub engine (tests/rr_root_diagnostics_engine_stub.py) and on the HIP
engine (MI355X): the two tables it writes equal the frames of the host statement (``farkle_ii_amd.rr_root_diagnostics``) fed with the
states of a plain round robin of the same configuration, the report carries the summary, the engine's option is restored; and what
the flag refuses."""
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

from test_rr_inference_runner import BLOCK_GAMES, KNOBS, MAX_ATTEMPTS, ROOTS, _base, _config, _family  # noqa: E402  (the same family and settings)

FILES = ["root_decision_agreement.parquet", "root_pairwise_diagnostics.parquet", "round_robin.json", "round_robin_inference_pairs.parquet",
         "round_robin_inference_strategies.parquet", "round_robin_strategies.parquet"]
LOOSE = ("ordinary_d_low", "ordinary_d_high", "score_p_value", "holm_adjusted_p")


@pytest.fixture(params=["host-stub", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request):
    from farkle_ii_amd import engine as eng_mod

    eng_mod.set_engine(None)
    if request.param == "host-stub":
        import rr_root_diagnostics_engine_stub

        eng_mod.set_engine(rr_root_diagnostics_engine_stub.Engine(0))
    yield request.param
    eng_mod.set_engine(None)


def test_root_diagnostics_command_writes_the_frames_of_the_host_statement(engine, tmp_path):
    import pandas as pd

    import rr_inference_cases as ri_cases
    import rr_root_diagnostics_cases as cases
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import rr_root_diagnostics as rd
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.strategies import pack_strategies

    cfg_path = _config(tmp_path)
    chosen, ids_file = _family(cfg_path, tmp_path)
    ids = [int(s.strategy_id) for s in chosen]
    out = tmp_path / "rr"
    args = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--inference", "--root-diagnostics", "--out", str(out)]
    main(args)
    assert sorted(f.name for f in out.iterdir()) == FILES
    eng = eng_mod.get_engine()
    assert eng.get_option("rr_keep_roots") == 0  # restored
    # a plain round robin of the same configuration, and the host statement over its states
    table = pack_strategies(chosen)
    states = [eng.h2h_round_robin(table, root, BLOCK_GAMES, MAX_ATTEMPTS)[0] for root in ROOTS]
    host = rd.diagnose(8, states, ROOTS, [BLOCK_GAMES] * 2, [MAX_ATTEMPTS] * 2, **KNOBS)
    cases.assert_margins(host, KNOBS["family_alpha"])
    want = rd.root_pairs_frame(host["rows"], host["roots"], ids, family_alpha=KNOBS["family_alpha"])
    got = pd.read_parquet(out / "root_pairwise_diagnostics.parquet")
    assert list(got.columns) == list(want.columns) and len(got) == 56 and got["root_seed"].tolist()[:2] == ROOTS
    exact = [c for c in want.columns if c not in LOOSE]
    pd.testing.assert_frame_equal(got[exact], want[exact], check_dtype=False, check_exact=True)
    for name in LOOSE[:2]:  # the halved bounds, as tests/test_rr_root_diagnostics_gpu.py holds them
        assert np.nanmax(np.abs(got[name].to_numpy() - want[name].to_numpy())) <= 1.25e-12
    tested = want["pair_inferentially_viable"].to_numpy()
    z = np.abs(want["score_z"].to_numpy()[tested])
    for name in LOOSE[2:]:  # Holm's products and maxima carry the p-values' relative distance
        g, w = got[name].to_numpy()[tested], want[name].to_numpy()[tested]
        assert (np.abs(g - w) <= ri_cases.p_value_bound(z).max() * w).all(), name
    agreement = pd.read_parquet(out / "root_decision_agreement.parquet")
    pd.testing.assert_frame_equal(agreement, rd.agreement_frame(host["agreement"], host["roots"], ids), check_dtype=False, check_exact=True)
    assert agreement["agreement_available"].any()
    report = json.loads((out / "round_robin.json").read_text())["root_diagnostics"]
    assert report["roots"] == ROOTS and (report["row_begin"], report["row_end"]) == (0, 28)
    assert report["summary"] == {name: int(v) for name, v in zip(rd.SUMMARY_COLS, host["summary"])}
    assert report["max_abs_discrepancy"] == host["max_abs_discrepancy"]
    assert report["root_specific_h2h_stability"] == rd.stability_summary(host["summary"])
    # a slice of the rows
    main([*args, "--rows", "5:9", "--force"])
    part = pd.read_parquet(out / "root_pairwise_diagnostics.parquet")
    pd.testing.assert_frame_equal(part, got.iloc[10:18].reset_index(drop=True), check_exact=True)
    pd.testing.assert_frame_equal(pd.read_parquet(out / "root_decision_agreement.parquet"), agreement.iloc[5:9].reset_index(drop=True), check_exact=True)
    assert json.loads((out / "round_robin.json").read_text())["root_diagnostics"]["summary"] == report["summary"]


def test_root_diagnostics_option_refusals(tmp_path):
    """Refused while reading the command line and the configuration: no engine is asked for."""
    from farkle_ii_amd.cli import main

    cfg_path = _config(tmp_path)
    _, ids_file = _family(cfg_path, tmp_path)
    base = [*_base(cfg_path), "--strategy-ids", str(ids_file), "--out", str(tmp_path / "never")]
    with pytest.raises(SystemExit, match="--root-diagnostics belongs to --inference"):
        main([*base, "--root-diagnostics"])

    def with_roots(roots):
        return [(f"sim.seed_list={roots}" if a == f"sim.seed_list={ROOTS}" else a) for a in base] + ["--inference", "--root-diagnostics"]

    with pytest.raises(SystemExit, match="--root-diagnostics: the root diagnostics admit one or two roots, got 3"):
        main(with_roots([42, 43, 44]))
    with pytest.raises(SystemExit, match="--root-diagnostics: the roots must be distinct"):
        main(with_roots([42, 42]))
    assert not (tmp_path / "never").exists()
