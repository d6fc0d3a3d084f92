"""Every kernel that runs behind the game kernel, on the MI355X, fed with the decided-outcome tables of `decided_table_cases.py`
(`test_decided_tables_cpu.py` states what each of them produces): batches without one completed game, all wins on one strategy at
a slice edge of ``fk_tally_reduce_kernel``, mirrored pairs whose P1-win difference is ``+paired``, ``-paired`` or undefined,
strategies that never win and never score next to one that wins whatever it completes, event lists of every completed game, second
scores of 0 throughout, column images whose nullable fields are all null.  Exact equality with the CPU oracle's statement of each
stage everywhere."""
from __future__ import annotations

import numpy as np
import pytest

import decided_table_cases as dc
from rare_events_engine_stub import Engine as RareStub
from seat_analysis_engine_stub import Engine as SeatStub
from test_rare_events_gpu import _same as same_rare_events

from farkle_ii_amd import game_stats as gs
from farkle_ii_amd import seat_analysis as sa

pytestmark = pytest.mark.gpu

IDS64 = ((np.arange(64, dtype=np.int64) * 37 + 11) % 257).astype(np.int32)  # unique, not in table order
COLUMNS_RANGE = dict(shuffle_begin=0, shuffle_end=40, shuffles_per_batch=16)
WIDE_PAIRS = dict(shuffle_begin=0, shuffle_end=320, shuffles_per_batch=32)  # more shuffles than the smallest workspace holds


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


class _Stub(RareStub, SeatStub):
    pass


@pytest.fixture(scope="module")
def want():
    """The oracle's statement of a run, computed once per distinct request of the module."""
    stub, memo = _Stub(), {}

    def get(method: str, name, k: int, *args, **kw):
        key = (method, name, k, repr(args), repr(sorted(kw.items())))
        if key not in memo:
            memo[key] = dc.run(stub, method, _table(name), k, *args, **kw)
        return memo[key]

    return get


def _table(name) -> np.ndarray:
    return dc.edge_table(name) if isinstance(name, int) else dc.table(name)


class _option:
    """``set_option`` for the length of a block; the engine's default afterwards."""
    DEFAULTS = {"chunk_bytes": 48 << 30, "use_lds_tally": -1, "columns_by_seat": -1, "game_stats_window": 0}

    def __init__(self, eng, name: str, value: int):
        self.eng, self.name, self.value = eng, name, value

    def __enter__(self):
        self.eng.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.eng.set_option(self.name, self.DEFAULTS[self.name])


# -- 1. tally routes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("winner", dc.EDGE_WINNERS)
def test_hip_tally_reduce_with_all_wins_on_a_slice_edge(eng, want, winner):
    w = want("tournament", winner, 2, **dc.EDGE_RANGE)["tally"]
    got = dc.run(eng, "tournament", dc.edge_table(winner), 2, **dc.EDGE_RANGE)["tally"]
    assert np.array_equal(got, w)
    assert got[:, winner, dc.WINS].sum() == got[..., dc.WINS].sum() > 0
    if winner == 896:  # chunks that cut the all-safety batches
        with _option(eng, "chunk_bytes", 1 << 20):
            chunked = dc.run(eng, "tournament", dc.edge_table(winner), 2, **dc.EDGE_RANGE)["tally"]
            launches = eng.timing()["play_launches"]
        assert launches >= 2
        assert np.array_equal(chunked, w)


@pytest.mark.parametrize("name,k", [("none64", 2), ("none64", 4), ("one64", 2)])
@pytest.mark.parametrize("lds_tally", [-1, 0])
def test_hip_tally_of_batches_without_a_completed_game(eng, want, name, k, lds_tally):
    for rng in (dc.TALLY_BATCHED, dict(dc.TALLY_BATCHED, shuffles_per_batch=None)):
        w = want("tournament", name, k, **rng)["tally"]
        with _option(eng, "use_lds_tally", lds_tally):
            got = dc.run(eng, "tournament", dc.table(name), k, **rng)["tally"]
        assert np.array_equal(got, w), rng
        if name == "none64":  # completed = in_batch - safety at safety == in_batch
            assert not got[..., dc.COMPLETED].any() and np.array_equal(got[..., dc.SAFETY], got[..., dc.GAMES])


@pytest.mark.parametrize("name,k", [("one64", 2), ("half64", 2), ("half64", 4)])
def test_hip_all_player_columns_of_strategies_that_never_score(eng, want, name, k):
    w = want("tournament", name, k, **dc.TALLY_BATCHED, want_seat_stats=True)
    got = dc.run(eng, "tournament", dc.table(name), k, **dc.TALLY_BATCHED, want_seat_stats=True)
    assert np.array_equal(got["tally"], w["tally"]) and np.array_equal(got["seat_stats"], w["seat_stats"])
    assert got["seat_ratio_sums"].tobytes() == w["seat_ratio_sums"].tobytes()
    never = dc.never_banks(dc.table(name))
    assert got["seat_ratio_sums"][:, never].tobytes() == np.zeros((3, int(never.sum()), 4)).tobytes()  # +0.0, never -0.0


# -- 2. seat counts and mirrored pairs ----------------------------------------------------------------------------------------------

def _pairs(e, name, rng, **extra):
    ids = dc.half12_ids() if name == "half12" else IDS64
    return dc.run(e, "tournament_seat_counts", dc.table(name), 2, **{**rng, **extra}, strategy_ids=ids, want_mirrored=True)


def _same_pairs(got: dict, w: dict) -> None:
    assert np.array_equal(got["seat_counts"], w["seat_counts"]) and np.array_equal(got["tally"], w["tally"])
    assert np.array_equal(got["pair_index"], w["pair_index"]) and np.array_equal(got["pair_sums"], w["pair_sums"])


@pytest.fixture(scope="module")
def pairs_want():
    stub = SeatStub()
    return {(name, rng["shuffle_end"]): _pairs(stub, name, rng)
            for name, rng in (("half12", dc.HALF12_PAIRS), ("half64", dc.HALF64_PAIRS), ("none64", dc.HALF64_PAIRS), ("half64", WIDE_PAIRS))}


@pytest.mark.parametrize("name", ["half12", "half64", "none64"])
def test_hip_mirrored_pairs_of_decided_games(eng, pairs_want, name):
    rng = dc.HALF12_PAIRS if name == "half12" else dc.HALF64_PAIRS
    w = pairs_want[name, rng["shuffle_end"]]
    got = _pairs(eng, name, rng)
    _same_pairs(got, w)
    kinds = dc.pair_kinds(got["pair_sums"])
    if name == "none64":
        assert kinds["none_completed"] == len(got["pair_sums"]) > 0 and not got["pair_sums"][:, [0, 1, 2, 4, 5]].any()
    else:
        assert all(n >= 1 for n in kinds.values()), kinds


def test_hip_mirrored_pairs_of_decided_games_across_chunks_and_calls(eng, pairs_want):
    w = pairs_want["half12", 700]
    with _option(eng, "chunk_bytes", 1 << 20):  # (700 shuffles of six games fit the smallest workspace: one chunk all the same)
        _same_pairs(_pairs(eng, "half12", dc.HALF12_PAIRS), w)
        print("play launches, half12:", eng.timing()["play_launches"])
        wide = _pairs(eng, "half64", WIDE_PAIRS)  # here chunks cut the batches and the pairs' segments
        launches = eng.timing()["play_launches"]
    assert launches >= 2
    _same_pairs(wide, pairs_want["half64", 320])
    ids = dc.half12_ids()
    parts = [sa.MirroredPairs.from_engine(_pairs(eng, "half12", dc.HALF12_PAIRS, shuffle_begin=a, shuffle_end=b), ids)
             for a, b in ((0, 300), (300, 700))]
    merged, whole = parts[0].merge(parts[1]), sa.MirroredPairs.from_engine(w, ids)
    assert np.array_equal(merged.ids, whole.ids) and np.array_equal(merged.sums, whole.sums)


# -- 3. game stats and rare events --------------------------------------------------------------------------------------------------

RARE = dict(rare_target_score=dc.RARE_TARGET, thresholds=dc.DENSE_THRESHOLDS)


@pytest.mark.parametrize("name,k", [("half64", 2), ("half64", 4), ("none64", 4), ("one64", 2)])
def test_hip_rare_events_when_every_completed_game_is_one(eng, want, name, k):
    w = want("tournament_rare_events", name, k, **dc.HALF64_PAIRS, **RARE)
    got = dc.run(eng, "tournament_rare_events", dc.table(name), k, **dc.HALF64_PAIRS, **RARE)
    same_rare_events(got, w)
    completed = int(got["game_stats"]["game_counts"][gs.COMPLETED])
    assert got["rare_events"]["events"] >= completed and (completed == 0) == (name == "none64")
    if name != "half64":  # second scores of 0 in every game; the completed games a minority (one64: at most one a shuffle)
        assert got["rare_events"]["game_second"][1:].sum() == 0 and completed <= 96


def test_hip_game_stats_when_every_margin_spills(eng, want):
    w = want("tournament_rare_events", "half64", 2, **dc.HALF64_PAIRS, **RARE)
    with _option(eng, "game_stats_window", 8):  # margins and second scores of 400 points and more, rounds from 8: all through the spill list
        spilled = dc.run(eng, "tournament_rare_events", dc.table("half64"), 2, **dc.HALF64_PAIRS, **RARE)
        tiny = dc.run(eng, "tournament_rare_events", dc.table("half64"), 2, **dc.HALF64_PAIRS, **RARE, spill_capacity=1)
    completed = int(w["game_stats"]["game_counts"][gs.COMPLETED])
    print("spilled", spilled["spilled"], "completed games", completed)
    assert spilled["spilled"] > completed and tiny["spilled"] == spilled["spilled"] and tiny["attempts"] == 2
    same_rare_events(spilled, w)
    same_rare_events(tiny, w)


# -- 4. lags ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,rounds", [("one64", dc.MAX_ROUNDS), ("one64", dc.ONE64_ALWAYS_ROUNDS), ("none64", dc.MAX_ROUNDS)])
def test_hip_lag_sums_of_constant_and_one_sided_series(eng, want, name, rounds):
    w = want("tournament_lags", name, 2, 0, dc.LAG_SHUFFLES, dc.LAGS, max_rounds=rounds)
    got = dc.run(eng, "tournament_lags", dc.table(name), 2, 0, dc.LAG_SHUFFLES, dc.LAGS, max_rounds=rounds)
    for key in ("tally", "lag_sums", "lag_head", "lag_tail"):
        assert np.array_equal(got[key], w[key]), key
    win_cols = got["lag_sums"][:, :, [dc.LAG_WX, dc.LAG_WY, dc.LAG_WXY]]
    if name == "none64":  # every value is the round limit, never a win
        assert not win_cols.any() and np.all(got["lag_head"] == dc.MAX_ROUNDS) and np.all(got["lag_tail"] == dc.MAX_ROUNDS)
    else:
        assert win_cols[17].all() and not np.delete(win_cols, 17, axis=0).any()
        if rounds == dc.ONE64_ALWAYS_ROUNDS:  # a win in every shuffle: wx = wy = wxy = pairs
            assert np.array_equal(win_cols[17], np.repeat(got["lag_sums"][17, :, [dc.LAG_PAIRS]].T, 3, axis=1))


# -- 5. columns ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("none64", 2), ("none64", 4), ("half64", 2), ("half64", 4)])
@pytest.mark.parametrize("by_seat", [0, 1])
def test_hip_column_images_of_decided_games(eng, want, name, k, by_seat):
    w = want("tournament_columns", name, k, **COLUMNS_RANGE, strategy_ids=IDS64)
    with _option(eng, "columns_by_seat", by_seat):
        got = dc.run(eng, "tournament_columns", dc.table(name), k, **COLUMNS_RANGE, strategy_ids=IDS64)
    assert np.array_equal(got["tally"], w["tally"])
    gps = 64 // k
    defined = ((4 + 13 * k) * 4 + 2 + k) * gps  # (an image is padded to a multiple of 64 bytes; nothing reads the padding)
    assert got["columns"].shape == w["columns"].shape and got["columns"][:, :defined].tobytes() == w["columns"][:, :defined].tobytes()
    if name == "none64":  # winner, winning score, margin, every rank and loss margin: null, held as 0; status 1 in every game
        planes = got["columns"][:, :(4 + 13 * k) * 4 * gps].view(np.int32).reshape(40, 4 + 13 * k, gps)
        null = [0, 1, 2] + [4 + 13 * s + f for s in range(k) for f in (0, 5, 6)]  # (and every seat's score is 0)
        assert not planes[:, null].any() and np.all(planes[:, 3] == dc.MAX_ROUNDS)
        assert np.all(got["columns"][:, (4 + 13 * k) * 4 * gps:(4 + 13 * k) * 4 * gps + gps] == 1)
