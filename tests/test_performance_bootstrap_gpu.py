"""The performance stage's joint batch bootstrap on the MI355X: ``fk_performance_bootstrap`` through the C-ABI against the fixture (the
reference's own range writer and reduction) and against the NumPy host statement, every output bit for bit — replicate ranges split
at arbitrary points with the contrast sums carried, device blocks of every size, batch counts that differ per player count (1
included), strategy counts off the tile width, ``top_n`` at both ends, no controls, all-tied input, counts beyond 32 bits and
totals beyond 2**53 (no fast route guards the integer product: a 32-bit instance was measured and not kept), the bounded-draw probe where half the draws are rejected, the zero-exposure
error, a production-shaped call, and ``farkle run --performance-bootstrap`` on the HIP engine against the same run on the stub."""
from __future__ import annotations

import numpy as np
import pytest

import performance_bootstrap_cases as pc
from performance_bootstrap_engine_stub import Engine as StubEngine

from farkle_ii_amd import performance_bootstrap as pb
from farkle_ii_amd.backend import COORD_DTYPE, FK_ERR_ARG, FarkleHipError
from farkle_ii_amd.random import RandomPurpose, coordinate_seed_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c["name"])
def test_hip_fixture_cases_equal_the_reference(eng, case):
    matrices = pc.case_matrices(case)
    required = sorted(matrices)
    p = pb.project(matrices, required)
    want = pc.case_scores(case)
    for r in case["ranges"]:  # the range writer's payload
        got = eng.performance_bootstrap(case["root_seed"], p.required_k, p.wins, p.exposures, r["start"], r["stop"], 0, 0.0)
        assert got["scores"].tobytes() == want[r["start"]:r["stop"]].tobytes()
    for range_size in (None, case["range_size"], 7):
        boot, contrasts = pb.performance_bootstrap_tables(eng, matrices, required, case["replicates"], case["candidate_contribution_size"],
                                                          case["delta_across_k"], case["controls"], range_size=range_size)
        assert pc.encode(boot) == case["bootstrap"] and boot.schema.equals(pb.bootstrap_schema())
        assert pc.encode(contrasts) == case["contrasts"] and contrasts.schema.equals(pb.contrast_schema())


def _both(eng, args, **kw):
    return eng.performance_bootstrap(*args, **kw), pb.host_bootstrap(*args, **kw)


@pytest.mark.parametrize("S,batches", [(1, {2: 3}), (63, {2: 5, 3: 1}), (257, {2: 65, 4: 64, 6: 1, 7: 130}), (1000, {3: 33})],
                         ids=["S1", "S63_B1", "S257_tiles", "S1000"])
def test_hip_equals_the_host_statement(eng, S, batches):
    ks, wins, exposures = pc.synthetic(S, S, batches)
    controls = sorted({0, S // 2, S - 1})
    for top_n in (1, S, min(7, S)):
        got, want = _both(eng, (3, ks, wins, exposures, 5, 45, top_n, 0.02), controls=controls)
        pc.assert_same(got, want)
    got, want = _both(eng, (3, ks, wins, exposures, 0, 19, 2 if S > 1 else 1, 0.0))  # no controls
    pc.assert_same(got, want)
    assert got["contrast_sum"].shape == (0, S)
    empty = eng.performance_bootstrap(3, ks, wins, exposures, 4, 4, 1, 0.0, controls=controls)  # an empty range changes nothing
    assert empty["scores"].shape == (0, S) and not empty["rank_sum"].any() and not empty["contrast_sum"].any()


def test_hip_split_ranges_and_device_blocks_carry_the_sums(eng):
    ks, wins, exposures = pc.synthetic(8, 300, {2: 20, 3: 11, 5: 1})
    controls = [4, 299]
    args = (21, ks, wins, exposures)
    want = pb.host_bootstrap(*args, 0, 100, 25, 0.01, controls=controls)
    whole = eng.performance_bootstrap(*args, 0, 100, 25, 0.01, controls=controls)
    pc.assert_same(whole, want)
    for cuts in ((0, 1, 17, 18, 64, 100), (0, 50, 100), (0, 99, 100)):
        parts, csum, csq = [], None, None
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(eng.performance_bootstrap(*args, a, b, 25, 0.01, controls=controls, contrast_sum=csum, contrast_square_sum=csq))
            csum, csq = parts[-1]["contrast_sum"], parts[-1]["contrast_square_sum"]
        merged = {"scores": np.concatenate([p["scores"] for p in parts]), "contrast_sum": csum, "contrast_square_sum": csq}
        for name in ("rank_sum", "rank_square_sum", "top_counts", "shortlist_counts"):
            merged[name] = sum(p[name] for p in parts)
        pc.assert_same(merged, want)
    for block in (16, 32, 48):  # the device's own blocks of the range
        eng.set_option("bootstrap_block", block)
        try:
            pc.assert_same(eng.performance_bootstrap(*args, 0, 100, 25, 0.01, controls=controls), want)
        finally:
            eng.set_option("bootstrap_block", 0)
    sums = pb.run_bootstrap(eng, pb.Projection(21, tuple(ks), np.arange(300), wins, exposures, []), 100, 25, 0.01, controls, range_size=30)
    pc.assert_same({**want, "rank_sum": sums.rank_sum, "rank_square_sum": sums.rank_square_sum, "top_counts": sums.top_counts,
                    "shortlist_counts": sums.shortlist_counts, "contrast_sum": sums.contrast_sum,
                    "contrast_square_sum": sums.contrast_square_sum}, want, scores=False)


def test_hip_all_tied_input(eng):
    ks, wins, exposures = pc.synthetic(2, 1, {2: 6, 3: 4})
    wins = [np.repeat(w, 200, axis=1) for w in wins]  # 200 identical columns: every score of a replicate is the same
    exposures = [np.repeat(e, 200, axis=1) for e in exposures]
    got, want = _both(eng, (1, ks, wins, exposures, 0, 40, 10, 0.0), controls=[3])
    pc.assert_same(got, want)
    assert np.array_equal(got["rank_sum"], 40 * np.arange(1, 201)) and np.array_equal(got["shortlist_counts"], np.full(200, 40))
    assert got["top_counts"].tolist() == [40] * 10 + [0] * 190 and not got["contrast_sum"].any()


def test_hip_counts_beyond_32_bits(eng):
    ks, wins, exposures = pc.synthetic(4, 130, {2: 9, 4: 70})
    big_e = [e * (2 ** 33 + 12345) + 7 for e in exposures]
    big_w = [w * (2 ** 33 + 999) for w in wins]
    assert max(int(e.max()) for e in big_e) > 2 ** 32
    got, want = _both(eng, (77, ks, big_w, big_e, 0, 33, 5, 0.01), controls=[1])
    pc.assert_same(got, want)
    got, want = _both(eng, (77, ks, [wins[0], big_w[1]], [exposures[0], big_e[1]], 0, 33, 5, 0.01), controls=[1])  # one player count only
    pc.assert_same(got, want)
    wide = [np.full_like(e, 2 ** 55 + 3) for e in exposures]  # totals beyond 2**53: the int64 -> float64 conversion rounds as numpy's
    got, want = _both(eng, (77, ks, [w * 2 ** 50 + 1 for w in wins], wide, 0, 33, 5, 0.01), controls=[1])
    pc.assert_same(got, want)
    huge = [np.full_like(e, 2 ** 62) for e in exposures]  # a resampled total could pass 2**63: refused, not wrapped
    with pytest.raises(FarkleHipError) as err:
        eng.performance_bootstrap(77, ks, wins, huge, 0, 4, 5, 0.01)
    assert err.value.code == FK_ERR_ARG


@pytest.mark.parametrize("bound", [1, 2, 100, 4300, 2 ** 31 + 1, 2 ** 32 - 1])
def test_hip_bounded_draw_probe_equals_numpy(eng, bound):
    n, n_draws = (3000, 40) if bound == 2 ** 31 + 1 else (200, 64)
    coords = np.zeros(n, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"] = int(RandomPurpose.BOOTSTRAP), 2 ** 40 + 5, 1 + np.arange(n) % 12
    coords["replicate_index"] = np.arange(n) * 7
    got = eng.debug_bounded_draws(coords, bound, n_draws)
    want = np.stack([np.random.Generator(np.random.PCG64DXSM(coordinate_seed_sequence(
        RandomPurpose.BOOTSTRAP, root_seed=2 ** 40 + 5, k=int(c["k"]), replicate_index=int(c["replicate_index"])))).integers(
            0, bound, size=n_draws) for c in coords])
    assert np.array_equal(got.astype(np.int64), want)
    with pytest.raises(FarkleHipError):
        eng.debug_bounded_draws(coords[:1], 2 ** 32, 1)


def test_hip_zero_exposure_total_is_an_error(eng):
    ks, wins, exposures = pc.synthetic(6, 40, {2: 4, 3: 5})
    exposures[1][:, 17] = 0
    with pytest.raises(FarkleHipError, match="zero complete-support exposure") as err:
        eng.performance_bootstrap(5, ks, wins, exposures, 0, 20, 3, 0.0)
    assert err.value.code == FK_ERR_ARG
    exposures[1][:, 17] = 1  # ... and the context is usable afterwards
    got, want = _both(eng, (5, ks, wins, exposures, 0, 20, 3, 0.0))
    pc.assert_same(got, want)
    for bad in (dict(top_n=41), dict(controls=[40]), dict(replicate_end=-1)):
        kw = dict(replicate_end=20, top_n=3, controls=[])
        kw.update(bad)
        with pytest.raises(FarkleHipError):
            eng.performance_bootstrap(5, ks, wins, exposures, 0, kw["replicate_end"], kw["top_n"], 0.0, controls=kw["controls"])


def test_hip_production_shape_equals_the_host_statement(eng):
    ks, wins, exposures = pc.synthetic(12, 5160, {k: 100 for k in (2, 3, 4, 5, 6, 8, 10, 12)}, low=30, high=60)
    args = (20261016, ks, wins, exposures, 1000, 1256, 75, 0.03)
    got, want = _both(eng, args, controls=[0, 2580, 5159])
    pc.assert_same(got, want)


def test_farkle_run_on_the_hip_engine_equals_the_stub_run(tmp_path, monkeypatch):
    import pyarrow.parquet as pq

    import test_performance_bootstrap_runner as tr
    from farkle_ii_amd import engine as eng_mod
    from farkle_ii_amd import runner
    from farkle_ii_amd.cli import main
    from farkle_ii_amd.config import load_app_config

    monkeypatch.setattr(runner, "MAX_GAMES_PER_LAUNCH", 400)
    cfgs = {}
    for name, engine in (("stub", StubEngine(0)), ("hip", None)):
        eng_mod.set_engine(engine)
        try:
            path = tr._config(tmp_path, name=name)
            main(["--config", str(path), "run", "--performance-bootstrap"])
            cfgs[name] = load_app_config(path, seed_list_len=1)
        finally:
            eng_mod.set_engine(None)
    for k in tr.KS:
        assert np.load(cfgs["hip"].performance_batch_matrix_path(k)).tobytes() == np.load(cfgs["stub"].performance_batch_matrix_path(k)).tobytes()
    for path in ("performance_bootstrap_path", "performance_control_contrasts_path"):
        a, b = pq.read_table(getattr(cfgs["hip"], path)()), pq.read_table(getattr(cfgs["stub"], path)())
        assert a.schema.equals(b.schema) and a.equals(b) and a.num_rows > 0
