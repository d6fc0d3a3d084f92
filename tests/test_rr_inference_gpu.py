"""``fk_rr_inference`` on the MI355X against the host statement (``farkle_ii_amd.rr_inference.infer``): the synthetic family of
tests/rr_inference_cases.py, the p-values over the whole z range, a family of several sort and scan tiles, a resident range that does
not start at pair 0, a row slice; the resident round robin against ``fk_rr_counts_add`` of the states ``fk_h2h_round_robin`` returns;
every refusal with its message and a good call after it."""
from __future__ import annotations

import numpy as np
import pytest

import round_robin_engine_stub as stub
import rr_inference_cases as cases
from farkle_ii_amd import rr_inference as ri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


def _load(eng, table, roots, target, cap, **where):
    eng.rr_counts_reset()
    for st in roots:
        eng.rr_counts_add(table, st, target, cap, **where)


@pytest.fixture(scope="module")
def synthetic():
    n, roots, target, cap = cases.synthetic_family()
    counts = ri.combine_counts(roots, [target] * 2, [cap] * 2)
    host = {de: ri.infer(n, counts, delta_equivalence=de, **cases.PARAMS) for de in (None, cases.DELTA_EQUIVALENCE)}
    for de, h in host.items():
        cases.assert_margins(h, cases.PARAMS["practical_delta"], de, cases.PARAMS["family_alpha"])
    return stub.random_valid_table(n, 5), roots, target, cap, host


@pytest.mark.parametrize("equivalence", [None, cases.DELTA_EQUIVALENCE], ids=["equivalence_off", "equivalence_on"])
def test_synthetic_family(eng, synthetic, equivalence):
    table, roots, target, cap, host = synthetic
    _load(eng, table, roots, target, cap)
    dev = eng.rr_inference(delta_equivalence=equivalence, rows=(0, 66), **cases.PARAMS)
    cases.compare(dev, host[equivalence])
    rows = dev["rows"]
    assert (rows["score_p_value"][[2, 13, 23]] == 0.0).all() and rows["holm_order"][[2, 13, 23]].tolist() == [1, 2, 3]  # (0,3) (1,4) (2,5)
    ties = rows["holm_order"][[0, 1, 11, 30, 45]]                                                                     # the identical pairs
    assert len(set(rows["score_p_value"][[0, 1, 11, 30, 45]])) == 1 and (np.diff(ties) > 0).all()
    none = eng.rr_inference(delta_equivalence=equivalence, want_strategies=False, **cases.PARAMS)  # rows and strategy_classes are nullable
    assert none["rows"] is None and none["strategies"] is None and np.array_equal(none["class_counts"], dev["class_counts"])


def test_p_values_over_the_z_range(eng):
    """4 097 pairs whose z steps through 0 .. 37.5 (x_ab = N (1/2 + e), x_ba = N (1/2 - e), z = 2 e sqrt(2 N)), and 89 beyond 39."""
    n, games = 92, 2_000_000
    n_pairs = n * (n - 1) // 2
    e = np.minimum(np.arange(n_pairs) / 4096.0, 1.0) * 0.009375
    e[4097:] = np.linspace(0.0098, 0.5, n_pairs - 4097)  # |z| from 39 up to the N : 0 corner
    x_ab = np.rint(games * (0.5 + e)).astype(np.int64)
    st = np.zeros((n_pairs, 2, 5), dtype=np.uint32)
    st[:, 0] = np.stack([np.full(n_pairs, games), np.full(n_pairs, games), np.zeros(n_pairs, dtype=np.int64), x_ab, games - x_ab], axis=1)
    st[:, 1] = np.stack([np.full(n_pairs, games), np.full(n_pairs, games), np.zeros(n_pairs, dtype=np.int64), games - x_ab, x_ab], axis=1)
    _load(eng, stub.random_valid_table(n, 6), [st], games, games)
    dev = eng.rr_inference(rows=(0, n_pairs), **cases.PARAMS)
    host = ri.infer(n, ri.combine_counts([st], [games], [games]), intervals="bisection", **cases.PARAMS)
    z = np.abs(host["rows"]["score_z"])
    assert z[0] == 0.0 and 37.49 < z[4096] < 37.51 and (z[4097:] >= 39.0).all() and 0.005 < np.diff(z[:4097]).min() and np.diff(z[:4097]).max() < 0.015
    cases.assert_margins(host, cases.PARAMS["practical_delta"], None, cases.PARAMS["family_alpha"])
    from scipy.stats import norm

    p_ref, p_dev = 2.0 * norm.sf(z), dev["rows"]["score_p_value"]
    normal = p_ref >= 2.3e-308
    excess = np.abs(p_dev[normal] - p_ref[normal]) / p_ref[normal] * 2.0**52 - z[normal] ** 2
    print(f"device erfc against scipy over z = 0 .. 37.5: largest (relative distance / 2^-52 - z^2) = {excess.max():.3f} (allowed: 8)")
    cases.compare(dev, host)


@pytest.fixture(scope="module")
def wide():
    n, roots, target, cap = cases.random_family()
    counts = ri.combine_counts(roots, [target], [cap])
    host = ri.infer(n, counts, delta_equivalence=cases.DELTA_EQUIVALENCE, intervals="bisection", **cases.PARAMS)
    cases.assert_margins(host, cases.PARAMS["practical_delta"], cases.DELTA_EQUIVALENCE, cases.PARAMS["family_alpha"])
    return n, stub.random_valid_table(n, 8), roots, target, cap, counts, host


def test_scale_and_row_slice(eng, wide):
    """n = 300, 44 850 pairs: several sort and scan tiles, seven nonviable pairs; then a slice of the rows."""
    n, table, roots, target, cap, _, host = wide
    _load(eng, table, roots, target, cap)
    dev = eng.rr_inference(delta_equivalence=cases.DELTA_EQUIVALENCE, rows=(0, 44_850), **cases.PARAMS)
    assert dev["class_counts"][6] == 7 and (dev["strategies"][:, 11] == 0).sum() == 14
    cases.compare(dev, host)
    part = eng.rr_inference(delta_equivalence=cases.DELTA_EQUIVALENCE, rows=(12_345, 13_001), **cases.PARAMS)
    assert part["rows"].tobytes() == dev["rows"][12_345:13_001].tobytes()
    assert np.array_equal(part["class_counts"], dev["class_counts"]) and np.array_equal(part["strategies"], dev["strategies"])


def test_resident_range_that_starts_inside_the_table(eng, wide):
    n, table, roots, target, cap, counts, _ = wide
    lo, hi = 1_003, 9_130  # inside rows of the pair triangle on both sides
    _load(eng, table, [roots[0][lo:hi]], target, cap, pair_begin=lo, pair_end=hi)
    dev = eng.rr_inference(delta_equivalence=cases.DELTA_EQUIVALENCE, rows=(lo, hi), **cases.PARAMS)
    host = ri.infer(n, counts[lo:hi], pair_begin=lo, delta_equivalence=cases.DELTA_EQUIVALENCE, intervals="bisection", **cases.PARAMS)
    cases.assert_margins(host, cases.PARAMS["practical_delta"], cases.DELTA_EQUIVALENCE, cases.PARAMS["family_alpha"])
    assert dev["rows"]["pair_id"][0] == lo and dev["rows"]["pair_id"][-1] == hi - 1
    cases.compare(dev, host)


@pytest.mark.parametrize("window", [None, 32, 2])
def test_resident_round_robin_against_counts_add(eng, window):
    """DESIGN 5.10's hard case, roots 11 and 12: the resident entry keeps the states on the device; the inference over them is bit-equal
    to the inference over fk_rr_counts_add of the states fk_h2h_round_robin returns, the summary is today's, and a refused call in
    between leaves the accumulator untouched."""
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    table = stub.hard_table()
    call = {k: v for k, v in stub.HARD.items() if k != "root_seed"}
    knobs = dict(family_alpha=0.02, practical_delta=0.03, delta_equivalence=0.25, min_candidate_completion_rate=0.5)
    saved = eng.get_option("rr_window_blocks")
    try:
        if window is not None:
            eng.set_option("rr_window_blocks", window)
        plain = [eng.h2h_round_robin(table, root_seed=root, **call) for root in (11, 12)]
        eng.rr_counts_reset()
        summary = eng.h2h_round_robin_resident(table, root_seed=11, **call)
        with pytest.raises(FarkleHipError, match="table, range or family differs") as refused:
            eng.h2h_round_robin_resident(table, root_seed=12, pair_end=60, **call)
        assert refused.value.code == FK_ERR_ARG
        with pytest.raises(FarkleHipError, match="target must be in"):
            eng.h2h_round_robin_resident(table, root_seed=12, target=75, max_attempts=74, max_rounds=24)
        eng.h2h_round_robin_resident(table, root_seed=12, summary=summary, **call)
        resident = eng.rr_inference(rows=(0, 66), **knobs)
    finally:
        eng.set_option("rr_window_blocks", saved)
    assert np.array_equal(summary, plain[0][1] + plain[1][1])
    _load(eng, table, [plain[0][0], plain[1][0]], call["target"], call["max_attempts"])
    added = eng.rr_inference(rows=(0, 66), **knobs)
    assert resident["rows"].tobytes() == added["rows"].tobytes()
    assert np.array_equal(resident["class_counts"], added["class_counts"]) and np.array_equal(resident["strategies"], added["strategies"])
    counts = ri.combine_counts([plain[0][0], plain[1][0]], [call["target"]] * 2, [call["max_attempts"]] * 2)
    assert np.array_equal(resident["rows"]["games_attempted"], counts[:, :, 0].sum(axis=1))
    tested = (resident["rows"]["flags"] & 1) != 0
    assert 0 < tested.sum() < 66 and not tested[0]  # rows 0 and 1 never bank: their pair completes no game
    host = ri.infer(12, counts, **knobs)
    cases.assert_margins(host, knobs["practical_delta"], knobs["delta_equivalence"], knobs["family_alpha"])
    cases.compare(resident, host)


def test_refusals_name_their_reason_and_leave_the_context_usable(eng, synthetic):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    table, roots, target, cap, host = synthetic
    eng.rr_counts_reset()
    with pytest.raises(FarkleHipError, match="no resident counts") as err:
        eng.rr_inference(**cases.PARAMS)
    assert err.value.code == FK_ERR_ARG
    _load(eng, table, roots, target, cap)
    want = host[None]["class_counts"]

    def good():
        assert np.array_equal(eng.rr_inference(**cases.PARAMS)["class_counts"], want)

    good()
    for bad, match in ((dict(rows=(0, 67)), "row range"), (dict(rows=(70, 80)), "row range"), (dict(family_alpha=0.0), "family_alpha must be in"),
                       (dict(family_alpha=1.0), "family_alpha must be in"), (dict(practical_delta=0.0), "practical_delta must be positive"),
                       (dict(delta_equivalence=0.0), "delta_equivalence must be in"), (dict(delta_equivalence=1.0), "delta_equivalence must be in"),
                       (dict(min_candidate_completion_rate=-0.1), "min_candidate_completion_rate must be in"),
                       (dict(min_candidate_completion_rate=1.01), "min_candidate_completion_rate must be in"),
                       (dict(family_pair_count=65), "is smaller than the 66 pairs"), (dict(family_pair_count=67), "fixed with the resident counts")):
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.rr_inference(**{**cases.PARAMS, **bad})
        assert err.value.code == FK_ERR_ARG, bad
        good()
    # the adding entries: what was fixed with the first call holds for the next
    for bad, match in ((dict(pair_end=65), "table, range or family differs"), (dict(family_pair_count=70), "table, range or family differs"),
                       (dict(family_pair_count=10), "family_pair_count 10 is smaller")):
        states = roots[0][: bad.get("pair_end", 66)]
        with pytest.raises(FarkleHipError, match=match):
            eng.rr_counts_add(table, states, target, cap, **bad)
        good()
    other = table.copy()
    other["score_threshold"][3] += 50
    with pytest.raises(FarkleHipError, match="table, range or family differs"):
        eng.rr_counts_add(other, roots[0], target, cap)
    broken = roots[0].copy()
    broken[7, 1, 3] += 1  # wins that do not add up to the completed games
    with pytest.raises(FarkleHipError, match="block_state of pair 7, order 1"):
        eng.rr_counts_add(table, broken, target, cap)
    good()
