"""Tournaments of 13 to 128 seats on the MI355X (``wide_table_cases.py``: one case per player count at which the launch plan, the
record layout, the rows tile or the column kernel changes, every case with completed and safety-limit games and wins at both
ends of the table), every entry point that plays them, and the refusal beyond 128 seats.  Every comparison is bytes or integers
equal, against the CPU oracle and the oracle-backed stubs."""
from __future__ import annotations

import numpy as np
import pytest

import wide_table_cases as wt
from matchup_engine_stub import Engine as MatchupStub
from oracle_engine_stub import Engine as OracleStub
from oracle_engine_stub import po
from rare_events_engine_stub import Engine as RareStub
from seat_analysis_engine_stub import Engine as SeatStub
from test_game_stats_gpu import _same as _same_game_stats
from test_rare_events_gpu import _same as _same_rare_events
from test_seat_analysis_gpu import _same_counts

from farkle_ii_amd.backend import COORD_DTYPE, FK_ERR_ARG, OVERRIDE_DTYPE, FarkleHipError, row_dtype

pytestmark = pytest.mark.gpu

DEFAULTS = {"lean": -1, "state_store": -1, "use_lds_tally": -1, "chunk_bytes": 48 << 30, "rows_chunk_games": 4_000_000, "columns_by_seat": -1}
LIMIT_MESSAGE = "at most 128 seats"


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    e = get_engine()
    yield e
    for name, value in DEFAULTS.items():
        e.set_option(name, value)


class _options:
    """Engine options for the length of a ``with`` block."""

    def __init__(self, eng, **values):
        self.eng, self.values = eng, values

    def __enter__(self):
        for name, value in self.values.items():
            self.eng.set_option(name, value)

    def __exit__(self, *exc):
        for name in self.values:
            self.eng.set_option(name, DEFAULTS[name])


def _same(got: dict, k: int, what, rows=True, perms=False, stats=False) -> None:
    """The parts of a tournament result that were asked for equal the oracle's result of case k."""
    want = wt.want(k)
    assert np.array_equal(got["tally"], want["tally"]), ("tally", k, what)
    if perms:
        assert np.array_equal(got["perms"], want["perms"]), ("perms", k, what)
    if rows:
        assert got["rows"].dtype.itemsize == want["rows"].dtype.itemsize == 4 + 28 * k
        assert got["rows"].tobytes() == want["rows"].tobytes(), ("rows", k, what)
    if stats:
        assert np.array_equal(got["seat_stats"], want["seat_stats"]), ("seat_stats", k, what)
        assert got["seat_ratio_sums"].tobytes() == want["seat_ratio_sums"].tobytes(), ("seat_ratio_sums", k, what)  # bit patterns


def _ran(eng, k: int, p: dict) -> None:
    """The last launch ran the instance the restated plan ``p`` names: an LDS-record / state-store instance of ``fk_play_kernel``
    (never a hot / cold one) of that block, record layout and LDS size."""
    args = wt.instance_args(eng.last_play_instance())
    timing = eng.timing()
    print(k, eng.last_play_instance(), {key: timing[key] for key in ("play_block", "play_grid", "play_lds_bytes", "play_launches")})
    assert (int(args[0]), args[1], args[4], args[5]) == (p["block"], str(p["lean"]).lower(), str(p["gs"]).lower(), "false")
    assert timing["play_block"] == p["block"] and timing["play_lds_bytes"] == p["lds"]


# ------------------------------------------------------------------------------------- 1. tournament parity per player count
@pytest.mark.parametrize("k", wt.KS)
def test_default_plan_equals_the_oracle_on_its_own_instance(eng, k):
    fig = wt.check_preconditions(k)
    got = eng.tournament(wt.table(k), k, want_rows=True, want_perms=True, want_seat_stats=True, **wt.call(k))
    print(k, fig)
    _same(got, k, "default", perms=True, stats=True)
    p = wt.plan(k, wt.table_size(k))
    _ran(eng, k, p)
    c = wt.constants()
    timing = eng.timing()
    assert (wt.instance_args(eng.last_play_instance())[4] == "true") == (k >= 65)  # the state-store instance from 65 seats on
    if k <= 64:
        assert timing["play_lds_bytes"] == timing["play_block"] * k * (c["FULL_BYTES"] if k in (33, 37) else c["LEAN_BYTES"])
    assert (timing["play_lds_bytes"] == 163_840) == (k in (16, 32, 64))
    assert timing["games"] == fig["games"]


@pytest.mark.parametrize("k", wt.KS)
def test_counts_only_calls_in_batches_and_as_one_batch(eng, k):
    t, kw = wt.table(k), wt.call(k)
    got = eng.tournament(t, k, **kw)
    _same(got, k, "counts only", rows=False)
    _ran(eng, k, wt.plan(k, wt.table_size(k)))
    total = wt.want(k)["tally"].sum(axis=0)
    one = eng.tournament(t, k, **dict(kw, shuffles_per_batch=None))
    assert one["tally"].shape[0] == 1 and np.array_equal(one["tally"][0], total), (k, "one batch")
    _ran(eng, k, wt.plan(k, wt.table_size(k), single_batch=True))  # an LDS tally wherever one fits beside the records
    with _options(eng, use_lds_tally=0):
        rec = eng.tournament(t, k, **dict(kw, shuffles_per_batch=None))
        _ran(eng, k, wt.plan(k, wt.table_size(k)))
    assert np.array_equal(rec["tally"][0], total), (k, "one batch through result records")


@pytest.mark.parametrize("k", wt.KS)
def test_calls_cut_into_at_least_three_chunks(eng, k):
    """The smallest workspace (1 MiB: three chunks and more from 64 seats on; at 128 seats for a counts-only call too, whose
    state-store instance needs the seat records whatever is asked for) and, for the tables it holds whole, rows-mode chunks of a
    third of the games."""
    gps, n_sh = wt.table_size(k) // k, wt.n_shuffles(k)
    with _options(eng, chunk_bytes=1 << 20, rows_chunk_games=gps * (n_sh // 3 - 1)):
        got = eng.tournament(wt.table(k), k, want_rows=True, want_perms=True, want_seat_stats=True, **wt.call(k))
        launches = eng.timing()["play_launches"]
        if k == 128:
            counts = eng.tournament(wt.table(k), k, **wt.call(k))
            assert eng.timing()["play_launches"] >= 3, (k, "counts only")
            _same(counts, k, "chunked counts", rows=False)
    print(k, "play_launches", launches)
    assert launches >= 3
    _same(got, k, "chunked", perms=True, stats=True)


@pytest.mark.parametrize("k", wt.KS)
def test_both_record_layouts_and_the_state_store(eng, k):
    t, kw = wt.table(k), wt.call(k)
    for lean in (0, 1):
        with _options(eng, lean=lean):
            got = eng.tournament(t, k, want_rows=True, **kw)
            p = wt.plan(k, wt.table_size(k), lean=lean)
            _ran(eng, k, p)
        _same(got, k, ("lean", lean))
        if k <= 37:  # both layouts fit
            assert not p["gs"] and p["lean"] == bool(lean)
        elif lean == 0:  # full records do not fit: the state-store instance (38: the first such count)
            assert p["gs"]
    with _options(eng, state_store=1):
        got = eng.tournament(t, k, want_rows=True, want_seat_stats=True, **kw)
        args = wt.instance_args(eng.last_play_instance())
        assert (args[0], args[4]) == ("768", "true")
        one = eng.tournament(t, k, **dict(kw, shuffles_per_batch=None))
    _same(got, k, "state store", stats=True)
    assert np.array_equal(one["tally"][0], wt.want(k)["tally"].sum(axis=0)), (k, "state store, one batch")


# ----------------------------------------------------------------------------------------- 2. a target beyond lean records
def test_target_beyond_lean_records_plays_on_full_records_or_is_refused(eng):
    """``target_score`` one point above what lean records carry, three rounds: every game ends at the limit.  37 seats are the
    last whose full records fit; 38 have no instance, and the context plays the next call as if nothing had happened."""
    kw = dict(root_seed=wt.ROOT, shuffle_begin=wt.BEGIN, shuffle_end=wt.BEGIN + 40, shuffles_per_batch=wt.SPB, target_score=wt.BEYOND_LEAN,
              max_rounds=3)
    t = wt.table(37)
    ref = po.tournament(t.view(po.STRATEGY_DTYPE), 37, wt.ROOT, wt.BEGIN, wt.BEGIN + 40, shuffles_per_batch=wt.SPB, target_score=wt.BEYOND_LEAN,
                        max_rounds=3, want_rows=True, want_perms=True)
    assert np.all(ref["rows"]["status"] == 1) and np.all(ref["rows"]["n_rounds"] == 3)
    got = eng.tournament(t, 37, want_rows=True, want_perms=True, **kw)
    _ran(eng, 37, dict(block=64, lean=False, gs=False, lds=64 * 37 * wt.constants()["FULL_BYTES"]))
    assert np.array_equal(got["tally"], ref["tally"]) and np.array_equal(got["perms"], ref["perms"])
    assert got["rows"].tobytes() == ref["rows"].tobytes()
    with pytest.raises(FarkleHipError, match="no kernel instance") as err:
        eng.tournament(wt.table(38), 38, want_rows=True, **kw)
    assert err.value.code == FK_ERR_ARG
    coords = np.zeros(2, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"], coords["game_index"] = 103, wt.ROOT, 38, [0, 1]
    with pytest.raises(FarkleHipError, match="no kernel instance") as err:
        eng.play_games(coords, wt.table(38), np.tile(np.arange(38, dtype=np.int32), 2), 38, target_score=wt.BEYOND_LEAN, max_rounds=3)
    assert err.value.code == FK_ERR_ARG
    _same(eng.tournament(wt.table(38), 38, want_rows=True, **wt.call(38)), 38, "after the refusal")


# ----------------------------------------------------------------------------------------------------- 3. the rows kernels
@pytest.mark.parametrize("k", [13, 19, 37])
def test_rows_kernels_into_pageable_and_pinned_buffers(eng, k):
    """The 128-lane tile, the 64-lane tile and the kernel without a tile, in one chunk and in chunks that end inside a block of
    the rows launch, into a pageable and into a page-locked buffer."""
    assert wt.rows_tile_lanes(k) == {13: 128, 19: 64, 37: 0}[k]
    t, kw = wt.table(k), wt.call(k)
    gps, n = wt.table_size(k) // k, len(wt.want(k)["rows"])
    for chunk in (4_000_000, gps * 7):
        with _options(eng, rows_chunk_games=chunk):
            got = eng.tournament(t, k, want_rows=True, **kw)
            pinned = eng.pinned_empty(n + 3, row_dtype(k))
            pinned.view(np.uint8)[:] = 0xA5
            again = eng.tournament(t, k, want_rows=True, rows_out=pinned, **kw)
        _same(got, k, ("pageable", chunk))
        _same(again, k, ("pinned", chunk))
        assert np.shares_memory(again["rows"], pinned) and np.all(pinned[n:].view(np.uint8) == 0xA5)  # nothing beyond the last row


# ---------------------------------------------------------------------------------------------------- 4. the column images
def _defined(columns: np.ndarray, k: int, gps: int) -> np.ndarray:
    return columns[:, :((4 + 13 * k) * 4 + 2 + k) * gps]  # (an image is padded to a multiple of 64 bytes; nothing reads the padding)


@pytest.mark.parametrize("k", wt.COLUMN_KS)
def test_column_images_equal_the_stub(eng, k):
    t, kw, gps = wt.table(k), wt.call(k), wt.table_size(k) // k
    ids = wt.ids(len(t))
    want = OracleStub().tournament_columns(t, k, strategy_ids=ids, **kw)
    assert np.array_equal(want["tally"], wt.want(k)["tally"])
    got = eng.tournament_columns(t, k, strategy_ids=ids, **kw)
    assert np.array_equal(got["tally"], want["tally"])
    assert np.array_equal(_defined(got["columns"], k, gps), _defined(want["columns"], k, gps)), (k, "auto")
    if k <= 16:  # one thread per (game, seat) by default; per game on request: the same bytes
        with _options(eng, columns_by_seat=0):
            per_game = eng.tournament_columns(t, k, strategy_ids=ids, **kw)
        assert np.array_equal(_defined(per_game["columns"], k, gps), _defined(want["columns"], k, gps)), (k, "per game")
        assert np.array_equal(per_game["tally"], want["tally"])


def test_column_images_are_refused_beyond_64_seats(eng):
    t = wt.table(65)
    with pytest.raises(FarkleHipError, match="column images hold tables of at most 64 seats") as err:
        eng.tournament_columns(t, 65, strategy_ids=wt.ids(len(t)), **wt.call(65))
    assert err.value.code == FK_ERR_ARG
    _same(eng.tournament(t, 65, want_rows=True, **wt.call(65)), 65, "after the refusal")


# ------------------------------------------------------------------------------------------------------- 5. the post-passes
@pytest.mark.parametrize("k", wt.POST_PASS_KS)
def test_game_stats_rare_events_and_lags_equal_their_stubs(eng, k):
    t, kw = wt.table(k), wt.call(k)
    want = RareStub().tournament_rare_events(t, k, thresholds=wt.RARE_THRESHOLDS, **kw)
    assert 0 < want["rare_events"]["events"] < wt.figures(k)["games"]
    rare = eng.tournament_rare_events(t, k, thresholds=wt.RARE_THRESHOLDS, want_seat_stats=True, **kw)
    _same_rare_events(rare, want)
    stats = eng.tournament_game_stats(t, k, want_seat_stats=True, **kw)
    _same_game_stats(stats, want)
    for res in (rare, stats):
        _same(res, k, "post-pass", rows=False, stats=True)
    histograms = eng.tournament_rare_events(t, k, want_events=False, **kw)
    assert histograms["rare_events"]["events"] == 0
    assert np.array_equal(histograms["rare_events"]["game_second"], rare["rare_events"]["game_second"])
    lags = (1, 2, 7)
    want_lags = OracleStub().tournament_lags(t, k, lags=lags, **kw)
    got_lags = eng.tournament_lags(t, k, lags=lags, **kw)
    for key in ("tally", "lag_sums", "lag_head", "lag_tail"):
        assert np.array_equal(got_lags[key], want_lags[key]), (k, key)
    assert want_lags["lag_sums"][:, :, 1].sum() > 0  # wins in the series


@pytest.mark.parametrize("k", [13, 15])
def test_seat_counts_of_thirteen_and_fifteen_seats(eng, k):
    t = wt.table(k) if k in wt.KS else wt.ki._random_legal(8 * k, 7 + k)
    kw = dict(root_seed=wt.ROOT, shuffle_begin=wt.BEGIN, shuffle_end=wt.BEGIN + 40, shuffles_per_batch=wt.SPB, max_rounds=14)
    want = SeatStub().tournament_seat_counts(t, k, **kw)
    got = eng.tournament_seat_counts(t, k, **kw)
    _same_counts(got, want)
    counts = want["seat_counts"]
    wins = counts[..., 0].sum(axis=(0, 1))
    assert counts.shape == (3, 8 * k, k, 3) and wins[0] >= 1 and wins[-1] >= 1 and (wins > 0).sum() >= k - 2  # wins at both ends of the table
    assert counts[..., 2].sum() >= k  # safety-limit exposures


# ------------------------------------------------------------------------------------------------------ 6. matchup records
@pytest.mark.parametrize("K", range(1, 17))
def test_matchup_records_of_every_instance(eng, K):
    """One template instance of the key kernel per seat count (its own sorting network; the BLAKE2b message holds 1 + max_players
    words, packed in pairs, so its last word's half depends on the parity), at every ``max_players`` of {K, 16, 31} it admits."""
    S = 6 * K
    t, ids = wt.ki._random_legal(S, 300 + K), wt.ids(S)
    assert np.any(np.diff(ids) < 0) and len(np.unique(ids)) == S  # not in table order
    stub = MatchupStub()
    kw = dict(lags=(1,), strategy_ids=ids, shuffles_per_batch=5, max_rounds=14)
    for mp in sorted({m for m in (K, 16, 31) if m >= K}):
        want = stub.tournament_matchups(t, K, 11, 2, 14, max_players=mp, **kw)
        got = eng.tournament_matchups(t, K, 11, 2, 14, max_players=mp, **kw)
        for key in ("digest", "seats", "rounds"):
            assert np.array_equal(got["matchups"][key], want["matchups"][key]), (K, mp, key)
        for key in ("tally", "lag_sums", "lag_head", "lag_tail"):
            assert np.array_equal(got[key], want[key]), (K, mp, key)
    parts = [eng.tournament_matchups(t, K, 11, b, e, max_players=mp, **kw)["matchups"] for b, e in ((2, 3), (3, 9), (9, 14))]
    for key in ("digest", "seats", "rounds"):  # (mp: the largest of the loop)
        assert np.array_equal(np.concatenate([p[key] for p in parts]), want["matchups"][key]), (K, "three calls", key)
    assert len(want["matchups"]["digest"]) == 12 * 6 and len(np.unique(want["matchups"]["rounds"])) > 1


# ----------------------------------------------------------------------------------------------------------- 7. game lists
@pytest.mark.parametrize("k", [13, 65, 128])
def test_game_lists_equal_the_oracle(eng, k):
    t = wt.table(k)
    n = 48
    rs = np.random.default_rng(500 + k)
    coords = np.zeros(n, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"] = 103, rs.integers(0, 2 ** 63, n), k
    coords["shuffle_index"], coords["game_index"] = rs.integers(0, 10 ** 6, n), rs.integers(0, 3000, n)
    seats = np.stack([rs.permutation(len(t))[:k] for _ in range(n)]).astype(np.int32)
    want = po.play_games(coords.view(po.COORD_DTYPE), t.view(po.STRATEGY_DTYPE), seats, k, max_rounds=wt.max_rounds(k), n_threads=4)
    got = eng.play_games(coords, t, seats, k, max_rounds=wt.max_rounds(k))
    assert (wt.instance_args(eng.last_play_instance())[4] == "true") == (k >= 65)
    assert got.tobytes() == want.tobytes()
    assert 0 < int((want["status"] == 0).sum()) < n  # both outcomes


# ------------------------------------------------------------------------------------------------------------ 8. the limit
def test_more_than_128_seats_are_refused_by_every_entry_that_plays_games(eng):
    """Written against the argument check: 129 seats never reach a kernel (128 equal the oracle in the tests above)."""
    k = wt.MAX_PLAYERS + 1
    t = wt.ki._random_legal(k, 1)
    ids = wt.ids(k)
    kw = dict(root_seed=wt.ROOT, shuffle_begin=0, shuffle_end=2, max_rounds=3)
    coords = np.zeros(1, dtype=COORD_DTYPE)
    coords["purpose"], coords["root_seed"], coords["k"] = 103, wt.ROOT, k
    tally = np.zeros((1, k, 26), dtype=np.int64)
    lead = eng._lead(np.ascontiguousarray(t), k, k, wt.ROOT, 0, 2, 2, 10_000, 3, np.zeros(0, dtype=OVERRIDE_DTYPE), tally)
    entries = {
        "fk_tournament_run": lambda: eng._check(eng._lib.fk_tournament_run(*lead, None, None)),
        "fk_tournament_run_stats": lambda: eng.tournament(t, k, want_seat_stats=True, want_seat_ratios=False, **kw),
        "fk_tournament_run_all_player": lambda: eng.tournament(t, k, want_seat_stats=True, **kw),
        "fk_tournament_run_columns": lambda: eng.tournament_columns(t, k, strategy_ids=ids, **kw),
        "fk_tournament_run_columns_seeds": lambda: eng.tournament_columns(t, k, strategy_ids=ids, shuffle_seeds_out=np.zeros(2, np.uint32), **kw),
        "fk_tournament_run_game_stats": lambda: eng.tournament_game_stats(t, k, **kw),
        "fk_tournament_run_rare_events": lambda: eng.tournament_rare_events(t, k, thresholds=(500,), **kw),
        "fk_tournament_run_lags": lambda: eng.tournament_lags(t, k, lags=(1,), **kw),
        "fk_play_games": lambda: eng.play_games(coords, t, np.arange(k, dtype=np.int32), k, max_rounds=3),
    }
    narrower = {  # entries whose own limit is below 128 keep it, and say so
        "fk_tournament_run_seat_counts": (lambda: eng.tournament_seat_counts(t, k, **kw), "1 .. 16 seats"),
        "fk_tournament_run_matchups": (lambda: eng.tournament_matchups(t, k, lags=(1,), strategy_ids=ids, max_players=31, **kw), "1 .. 16 seats"),
    }
    for name, run in entries.items():
        with pytest.raises(FarkleHipError, match=LIMIT_MESSAGE) as err:
            run()
        assert err.value.code == FK_ERR_ARG, name
        assert str(wt.MAX_PLAYERS) in str(err.value) and str(k) in str(err.value), name
    for name, (run, message) in narrower.items():
        with pytest.raises(FarkleHipError, match=message) as err:
            run()
        assert err.value.code == FK_ERR_ARG, name
    _same(eng.tournament(wt.table(13), 13, want_rows=True, want_seat_stats=True, **wt.call(13)), 13, "after the refusals", stats=True)


# ---------------------------------------------------------------------------------------------------------- 9. a wide fuzz
def test_fuzz_random_tables_of_13_to_64_seats(eng):
    """The randomized differential test of ``test_hip_parity.py`` (the same thresholds, targets and round limits) at 13 .. 64 seats
    with a seed of its own: rows, permutations and tallies bit-identical to the oracle."""
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    rs = np.random.default_rng(20_260_128)
    for trial in range(30):
        k = int(rs.integers(13, 65))
        S = k * int(rs.integers(1, 5))
        table = np.zeros(S, dtype=STRATEGY_DTYPE)
        for i in range(S):
            sf = int(rs.integers(0, 2))
            so = int(rs.integers(0, 2)) if sf else 0
            cs, cd = int(rs.integers(0, 2)), int(rs.integers(0, 2))
            rb = int(rs.integers(0, 2)) if (cs and cd) else 0
            table[i] = (int(rs.choice([0, 1, 49, 50, 51, 199, 250, 300, 500, 1000, 1001, 1350, 10_000])), int(rs.integers(-1, 7)), sf, so, cs, cd, rb,
                        int(rs.integers(0, 2)), int(rs.integers(0, 2)), int(rs.integers(0, 2)), 1000 + i)
        target = int(rs.choice([49, 100, 500, 1_234, 2000, 9_999, 10_000, 10_001, 20_000]))
        max_rounds = int(rs.choice([0, 1, 3, 50, 200, 300]))
        n_sh = int(rs.choice([1, 2, 7, 40]))
        root = int(rs.integers(0, 2**63))
        first = int(rs.integers(0, 2**40))
        got = eng.tournament(table, k, root, first, first + n_sh, shuffles_per_batch=3, target_score=target, max_rounds=max_rounds,
                             want_rows=True, want_perms=True)
        ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, root, first, first + n_sh, shuffles_per_batch=3, target_score=target,
                            max_rounds=max_rounds, want_rows=True, want_perms=True, n_threads=4)
        ctx = (trial, k, S, target, max_rounds, n_sh)
        assert np.array_equal(got["perms"], ref["perms"]), ctx
        assert got["rows"].tobytes() == ref["rows"].tobytes(), ctx
        assert np.array_equal(got["tally"], ref["tally"]), ctx
