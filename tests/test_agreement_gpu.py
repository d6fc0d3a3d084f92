"""``fk_agreement_pairs``, ``fk_rr_agreement`` and ``fk_rank_concordance`` on the MI355X against the host statements
(``farkle_ii_amd.structure_agreement``): every case of tests/agreement_cases.py with codes and counts byte-equal, codes null, and the
grid narrowed so that a small table takes several trips; Kendall's counts at the item counts where the tile walk changes shape; the
resident chain against the pair pass fed with the classes ``fk_rr_inference`` returns, equivalence on and off; every refusal with its
message and a good call after it; a partial resident range refused."""
from __future__ import annotations

import numpy as np
import pytest

import agreement_cases as cases
import round_robin_engine_stub as stub
import rr_inference_cases as ri_cases
from farkle_ii_amd import structure_agreement as sa
from farkle_ii_amd.backend import CONCORDANCE_MAX_M, CONCORDANCE_TILE

pytestmark = pytest.mark.gpu
T = CONCORDANCE_TILE


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.set_option("agreement_grid", 0)
    e.close()


def _inputs(name: str) -> tuple:
    c = cases.case(name)
    membership = sa.membership_from_frame(c["membership"], c["ids"])
    return c["n"], c["cls"], membership["win_rate_rank"], membership["trueskill_rank"]


@pytest.mark.parametrize("grid", [0, 1, 3], ids=["grid_default", "grid_1", "grid_3"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_pair_pass_against_the_host_statement(eng, name, grid):
    n, cls, win, ts = _inputs(name)
    codes = sa.pair_codes(n, cls, win, ts)
    counts = sa.pair_counts(codes, cls)
    eng.set_option("agreement_grid", grid)  # 276 pairs on one workgroup of 256: two trips; 11 175 on three: fifteen
    assert eng.get_option("agreement_grid") == grid
    try:
        dev = eng.agreement_pairs(n, cls, win, ts)
        assert dev["codes"].dtype == np.uint8 and dev["codes"].tobytes() == codes.tobytes()
        assert dev["counts"].tobytes() == counts.tobytes()
        bare = eng.agreement_pairs(n, cls, win, ts, want_codes=False)
        assert bare["codes"] is None and bare["counts"].tobytes() == counts.tobytes()
        t = eng.timing()
        assert 0.0 < t["perm_ms"] <= t["play_ms"] == t["total_ms"]
    finally:
        eng.set_option("agreement_grid", 0)


def _brute_force(x, y) -> list:
    """All i < j at once, by sign products (m up to a few hundred), or in row blocks."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    out = np.zeros(5, dtype=np.int64)
    for lo in range(0, len(x), 512):
        rows = np.arange(lo, min(lo + 512, len(x)))
        later = np.arange(len(x))[None, :] > rows[:, None]
        dx, dy = np.sign(x[rows, None] - x[None, :]), np.sign(y[rows, None] - y[None, :])
        out += [np.count_nonzero(later & (dx * dy > 0)), np.count_nonzero(later & (dx * dy < 0)), np.count_nonzero(later & (dx == 0) & (dy != 0)),
                np.count_nonzero(later & (dx != 0) & (dy == 0)), np.count_nonzero(later & (dx == 0) & (dy == 0))]
    return out.tolist()


# one tile cut by the diagonal; a full tile; a second, ragged tile row (diagonal, off-diagonal and ragged tiles); three tile rows
@pytest.mark.parametrize("m", [2, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("distinct", ["few", "many"])
def test_concordance_at_the_tile_edges(eng, m, distinct):
    rng = np.random.default_rng(1000 + m)
    top = 3 if distinct == "few" else 4 * m
    x, y = rng.integers(1, top + 1, size=m).astype(np.int32), rng.integers(1, top + 1, size=m).astype(np.int32)
    got = eng.rank_concordance(x, y)
    assert got.dtype == np.int64 and got.tolist() == _brute_force(x, y) == sa.concordance_counts(x, y).tolist()
    assert got.sum() == m * (m - 1) // 2 and (distinct == "many" or m == 2 or got[2:].min() > 0)
    t = eng.timing()
    assert t["play_ms"] == t["total_ms"] > 0.0


def test_concordance_of_equal_reversed_and_production_keys(eng):
    m = 2 * T + 1
    up = 1 + np.arange(m, dtype=np.int32)
    pairs = m * (m - 1) // 2
    assert eng.rank_concordance(np.full(m, 7, dtype=np.int32), np.full(m, 2 ** 31 - 1, dtype=np.int32)).tolist() == [0, 0, 0, 0, pairs]
    assert eng.rank_concordance(up, up[::-1]).tolist() == [0, pairs, 0, 0, 0]
    assert eng.rank_concordance(up, up).tolist() == [pairs, 0, 0, 0, 0]
    assert eng.rank_concordance(up, np.full(m, 1, dtype=np.int32)).tolist() == [0, 0, 0, pairs, 0]
    x, y = sa.scored_population(sa.membership_from_frame(cases.case("family_150")["membership"], cases.case("family_150")["ids"]))
    assert len(x) == 5156  # the 5 160 of the grid but those without one of the ranks
    got = eng.rank_concordance(x, y)
    assert got.tolist() == _brute_force(x, y)
    rng = np.random.default_rng(5160)
    x, y = rng.integers(1, 400, size=5160).astype(np.int32), rng.integers(1, 5161, size=5160).astype(np.int32)
    got = eng.rank_concordance(x, y)
    assert got.tolist() == _brute_force(x, y) and got[2] > 0 and got[4] > 0
    from scipy.stats import kendalltau

    assert np.float64(sa.kendall_from_counts(got, 5160)).tobytes() == np.float64(kendalltau(x, y).statistic).tobytes()


def _load(eng, table, roots, target, cap, **where):
    eng.rr_counts_reset()
    for st in roots:
        eng.rr_counts_add(table, st, target, cap, **where)


def _chain_against_stage(eng, n: int, win, ts, knobs: dict) -> dict:
    """``fk_rr_agreement`` over the resident counts against ``fk_agreement_pairs`` fed with the classes of ``fk_rr_inference``."""
    chain = eng.rr_agreement(win, ts, **knobs)
    t = eng.timing()
    assert t["play_ms"] == t["total_ms"] > 0.0 and 0.0 < t["perm_ms"] < t["play_ms"]
    inferred = eng.rr_inference(rows=(0, n * (n - 1) // 2), **knobs)
    cls = inferred["rows"]["decision_class"]
    stage = eng.agreement_pairs(n, cls, win, ts)
    assert chain["codes"].tobytes() == stage["codes"].tobytes() == sa.pair_codes(n, cls, win, ts).tobytes()
    assert chain["counts"].tobytes() == stage["counts"].tobytes()
    assert np.array_equal(chain["class_counts"], inferred["class_counts"])
    assert chain["counts"][1] == inferred["class_counts"][:4].sum() and chain["counts"][2] == inferred["class_counts"][5:].sum()
    assert chain["counts"][3] == inferred["class_counts"][6] and chain["counts"][4] == inferred["class_counts"][4]
    bare = eng.rr_agreement(win, ts, want_codes=False, **knobs)
    assert bare["codes"] is None and bare["counts"].tobytes() == chain["counts"].tobytes()
    return chain


def _ranks(n: int) -> tuple:
    rng = np.random.default_rng(n)
    win, ts = (1 + rng.permutation(n)).astype(np.int32), rng.integers(1, n // 2 + 1, size=n).astype(np.int32)
    win[3] = ts[5] = 0
    return win, ts


@pytest.mark.parametrize("equivalence", [None, ri_cases.DELTA_EQUIVALENCE], ids=["equivalence_off", "equivalence_on"])
def test_resident_chain_on_the_synthetic_family(eng, equivalence):
    n, roots, target, cap = ri_cases.synthetic_family()
    _load(eng, stub.random_valid_table(n, 5), roots, target, cap)
    chain = _chain_against_stage(eng, n, *_ranks(n), dict(delta_equivalence=equivalence, **ri_cases.PARAMS))
    assert chain["counts"][1] > 0 and chain["counts"][3] > 0 and (chain["counts"][4] > 0) == (equivalence is not None)
    assert 0 < chain["counts"][8] < chain["counts"][7] < chain["counts"][1]


def test_refusals_name_their_reason_and_leave_the_context_usable(eng):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    n, cls, win, ts = _inputs("every_class")
    codes = sa.pair_codes(n, cls, win, ts)

    def good():
        assert eng.agreement_pairs(n, cls, win, ts)["codes"].tobytes() == codes.tobytes()
        assert eng.rank_concordance([1, 2, 2], [3, 1, 1]).tolist() == [0, 2, 0, 0, 1]

    good()
    args = dict(n=n, decision_class=cls, win_rate_rank=win, trueskill_rank=ts)
    bad_class, bad_win, bad_ts = cls.copy(), win.copy(), ts.copy()
    bad_class[9] = 7
    bad_win[2], bad_ts[6] = -1, -(2 ** 31)
    empty = dict(decision_class=np.zeros(0, np.uint8), win_rate_rank=np.zeros(0, np.int32), trueskill_rank=np.zeros(0, np.int32))
    for bad, match in ((dict(n=1, **empty), "at least two strategies, got 1"), (dict(n=65537, **empty), "at most 2\\^31 - 1 pairs, 65537 strategies have 2147516416"),
                       (dict(decision_class=bad_class), "decision class 7 of pair 9"), (dict(win_rate_rank=bad_win), "row 2 has a negative rank \\(-1, "),
                       (dict(trueskill_rank=bad_ts), "row 6 has a negative rank")):
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.agreement_pairs(**{**args, **bad})
        assert err.value.code == FK_ERR_ARG, match
        good()
    lib, ctx = eng._lib, eng._ctx  # the null arrays: below the Python layer, which always hands arrays in
    import ctypes as C

    counts = np.zeros(11, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for call, match in ((lambda: lib.fk_agreement_pairs(ctx, C.c_int32(n), None, p(win), p(ts), None, p(counts)), "decision_class is required"),
                        (lambda: lib.fk_agreement_pairs(ctx, C.c_int32(n), p(cls), None, p(ts), None, p(counts)), "win_rate_rank, trueskill_rank and counts are required"),
                        (lambda: lib.fk_agreement_pairs(ctx, C.c_int32(n), p(cls), p(win), p(ts), None, None), "win_rate_rank, trueskill_rank and counts are required"),
                        (lambda: lib.fk_rank_concordance(ctx, C.c_int32(8), None, p(ts), p(counts)), "x, y and counts are required"),
                        (lambda: lib.fk_rank_concordance(ctx, C.c_int32(8), p(win), p(ts), None), "x, y and counts are required")):
        assert call() == FK_ERR_ARG and match in lib.fk_last_error(ctx).decode()
        good()
    one = np.ones(CONCORDANCE_MAX_M + 1, dtype=np.int32)
    for x, y, match in (([1], [1], "takes 2 to 65536 items .*, got 1"), (one, one, "takes 2 to 65536 items .*, got 65537"),
                        ([1, 0, 2], [1, 1, 1], "item 1 has the keys \\(0, 1\\): a key is at least 1"), ([1, 2, 3], [1, 1, -4], "item 2 has the keys \\(3, -4\\)")):
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.rank_concordance(x, y)
        assert err.value.code == FK_ERR_ARG, match
        good()
    # the resident chain: no counts, a partial range, bad ranks, the inference's own refusals; then a good call
    family, roots, target, cap = ri_cases.synthetic_family()
    table = stub.random_valid_table(family, 5)
    fwin, fts = _ranks(family)
    eng.rr_counts_reset()
    with pytest.raises(FarkleHipError, match="no resident counts") as err:
        eng.rr_agreement(fwin, fts, **ri_cases.PARAMS)
    assert err.value.code == FK_ERR_ARG
    _load(eng, table, [r[3:60] for r in roots], target, cap, pair_begin=3, pair_end=60)
    with pytest.raises(FarkleHipError, match=r"hold pairs \[3, 60\) of the table's 66: pair agreement needs the whole family") as err:
        eng.rr_agreement(fwin, fts, **ri_cases.PARAMS)
    assert err.value.code == FK_ERR_ARG
    _load(eng, table, roots, target, cap)
    negative = fwin.copy()
    negative[0] = -5
    for bad, match in ((dict(win_rate_rank=negative), "row 0 has a negative rank"), (dict(practical_delta=0.0), "practical_delta must be positive"),
                       (dict(family_alpha=1.0), "family_alpha must be in"), (dict(family_pair_count=67), "fixed with the resident counts")):
        with pytest.raises(FarkleHipError, match=match) as err:
            eng.rr_agreement(**{"win_rate_rank": fwin, "trueskill_rank": fts, **ri_cases.PARAMS, **bad})
        assert err.value.code == FK_ERR_ARG, match
    _chain_against_stage(eng, family, fwin, fts, dict(delta_equivalence=None, **ri_cases.PARAMS))
    good()
