"""A tournament call's request does not outlive the call.  Every ``fk_tournament_run*`` entry hands the engine one request value;
nothing of it stays in the context.  So after a call that fails late (a list that is too small: the whole range has been played) or
early (its argument checks), the next calls are what they were before it; every entry returns the plain call's tally over several
workspace chunks; and the same calls made in another order on the same engine return the same arrays.  Integer / byte equality
against the same library's plain call throughout (the oracle tests establish that one)."""
from __future__ import annotations

import numpy as np
import pytest

from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

pytestmark = pytest.mark.gpu

LAGS = (1, 2, 7)
IDS = ((np.arange(64, dtype=np.int64) * 37 + 11) % 257).astype(np.int32)  # unique, not in table order
LATE = dict(target_score=3000, max_rounds=9)  # some games end at the safety limit


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.engine import get_engine

    return get_engine()


@pytest.fixture(scope="module")
def table():
    from tools.time_config import table_for

    return table_for(64)


def _flat(result, prefix="") -> dict:
    out = {}
    for key, value in result.items():
        if isinstance(value, dict):
            out.update(_flat(value, f"{prefix}{key}."))
        else:
            out[prefix + key] = value
    return out


def _same(got: dict, want: dict, what: str) -> None:
    got, want = _flat(got), _flat(want)
    assert got.keys() == want.keys(), what
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {key}"
        else:
            assert g == w, f"{what}: {key}"


def _before(eng, table, k):
    return eng.tournament(table, k, 9, 0, 30, **LATE), eng.tournament_lags(table, k, 9, 0, 30, LAGS, **LATE)


def _clean(eng, table, k, before, what) -> None:
    plain, lags = before
    assert lags["tally"].tobytes() == plain["tally"].tobytes()
    _same(eng.tournament(table, k, 9, 0, 30, **LATE), plain, f"plain call after {what}")
    _same(eng.tournament_lags(table, k, 9, 0, 30, LAGS, **LATE), lags, f"lags call after {what}")


def test_after_a_call_that_fails_late_the_next_call_is_clean(eng, table):
    before = _before(eng, table, 4)
    with pytest.raises(FarkleHipError) as err:  # a threshold above every margin flags every completed game: four entries do not hold them
        eng.tournament_rare_events(table, 4, 9, 0, 30, rare_target_score=10 ** 6, thresholds=(-50, 2 ** 31 - 1), event_capacity=4,
                                   retry=False, **LATE)
    assert err.value.code == FK_ERR_ARG and err.value.events_needed > 4
    _clean(eng, table, 4, before, "the short event list")
    before = _before(eng, table, 2)
    with pytest.raises(FarkleHipError) as err:
        eng.tournament_seat_counts(table, 2, 9, 0, 30, strategy_ids=IDS, want_mirrored=True, pair_capacity=1, retry=False, **LATE)
    assert err.value.code == FK_ERR_ARG and err.value.pairs_needed > 1
    _clean(eng, table, 2, before, "the short pair list")


def test_after_a_call_that_fails_its_argument_checks_the_next_call_is_clean(eng, table):
    before = _before(eng, table, 4)
    with pytest.raises(FarkleHipError) as err:
        eng.tournament_seat_counts(table, 4, 9, 0, 30, strategy_ids=IDS, want_mirrored=True, **LATE)  # mirrored pairs exist at k = 2 only
    assert err.value.code == FK_ERR_ARG
    _clean(eng, table, 4, before, "the refused seat-count call")
    with pytest.raises(FarkleHipError) as err:
        eng.tournament_matchups(table, 4, 9, 0, 30, LAGS, IDS, 3, **LATE)  # max_players < k
    assert err.value.code == FK_ERR_ARG
    _clean(eng, table, 4, before, "the refused matchup call")


def _columns(eng, table, **kw):
    seeds = {"shuffle_seeds": np.zeros(600, dtype=np.uint32), "game_seeds": np.zeros(600 * 32, dtype=np.uint32)}
    out = eng.tournament_columns(table, 2, 42, 100, 700, IDS, shuffle_seeds_out=seeds["shuffle_seeds"], game_seeds_out=seeds["game_seeds"], **kw)
    return {**out, **seeds}


# every entry over k = 2, root 42, shuffles 100 .. 700 in batches of 50: the plain call first
ENTRIES = [
    ("plain", lambda e, t, **kw: e.tournament(t, 2, 42, 100, 700, **kw)),
    ("seat_stats", lambda e, t, **kw: e.tournament(t, 2, 42, 100, 700, want_seat_stats=True, **kw)),
    ("rows", lambda e, t, **kw: e.tournament(t, 2, 42, 100, 700, want_rows=True, **kw)),
    ("columns_seeds", _columns),
    ("lags", lambda e, t, **kw: e.tournament_lags(t, 2, 42, 100, 700, LAGS, **kw)),
    ("matchups", lambda e, t, **kw: e.tournament_matchups(t, 2, 42, 100, 700, LAGS, IDS, 12, **kw)),
    ("game_stats", lambda e, t, **kw: e.tournament_game_stats(t, 2, 42, 100, 700, **kw)),
    ("rare_events", lambda e, t, **kw: e.tournament_rare_events(t, 2, 42, 100, 700, thresholds=(500, 1000), **kw)),
    ("seat_counts", lambda e, t, **kw: e.tournament_seat_counts(t, 2, 42, 100, 700, strategy_ids=IDS, want_mirrored=True, **kw)),
]


@pytest.fixture(scope="module")
def chunked(eng, table):
    """Every entry's result with the smallest workspace (several chunks per call), and the plain call's launches."""
    eng.set_option("chunk_bytes", 1 << 20)
    try:
        results, launches = {}, None
        for name, call in ENTRIES:
            results[name] = call(eng, table, shuffles_per_batch=50)
            if name == "plain":
                launches = eng.timing()["play_launches"]
    finally:
        eng.set_option("chunk_bytes", 48 << 30)
    return results, launches


def test_every_entry_returns_the_plain_tally_over_several_chunks(chunked):
    results, launches = chunked
    assert launches >= 3
    plain = results["plain"]["tally"]
    assert plain.shape == (12, 64, plain.shape[2]) and plain.any()
    for name, result in results.items():
        assert result["tally"].dtype == plain.dtype and result["tally"].tobytes() == plain.tobytes(), name
    assert results["rare_events"]["rare_events"]["events"] > 0 and len(results["seat_counts"]["pair_sums"]) > 0  # the lists are not empty


def test_interleaving_leaves_no_residue(eng, table, chunked):
    results, _ = chunked
    for name, call in reversed(ENTRIES):  # the other order, one chunk per call
        _same(call(eng, table, shuffles_per_batch=50), results[name], name)
