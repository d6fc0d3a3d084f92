"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine (``oracle_engine_stub.Engine``) plus the two census calls, served from the roll
events of tests/trace_oracle.py (the oracle's game loop restated on its own primitives, pinned by ``row == the oracle's row``) with the
host statement of the census (``farkle_ii_amd.roll_census.RollCensus.from_events``)."""
from __future__ import annotations

import numpy as np
import pyoracle as po
import trace_oracle

from farkle_ii_amd.backend import CENSUS_TABLES, make_coords
from oracle_engine_stub import Engine as OracleEngine


def tournament_game_list(S: int, k: int, root_seed: int, shuffle_begin: int, shuffle_end: int):
    """(coords, seat_strategy) of the games a tournament plays for the range, in (shuffle, game) order: the permutation of namespace
    101 cut into tables of k, the seat streams of namespace 103 (src/farkle/simulation/run_tournament.py:301-351)."""
    gps = S // k
    shuffles = np.repeat(np.arange(shuffle_begin, shuffle_end, dtype=np.uint64), gps)
    games = np.tile(np.arange(gps, dtype=np.uint64), max(shuffle_end - shuffle_begin, 0))
    coords = make_coords(103, root_seed, k, shuffle_index=shuffles, game_index=games, n=len(games))
    seats = [po.permutation(po.coord(101, root_seed, k, sh), S)[:gps * k].reshape(gps, k) for sh in range(shuffle_begin, shuffle_end)]
    return coords, (np.concatenate(seats) if seats else np.zeros((0, k), np.int64)).astype(np.int32)


class Engine(OracleEngine):
    def census_games(self, coords, table, seat_strategy, k, target_score=10_000, max_rounds=200, turn_bins=256) -> dict:
        from farkle_ii_amd.roll_census import RollCensus

        ss = np.asarray(seat_strategy, dtype=np.int32).reshape(len(coords), k)
        _, begin, events = trace_oracle.pinned(coords, table, ss, k, target_score, max_rounds)
        census = RollCensus.from_events(events, begin, ss, len(table), turn_bins)
        return {name: getattr(census, name) for name in CENSUS_TABLES}

    def tournament_census(self, table, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch=None, target_score=10_000,
                          max_rounds=200, overrides=None, turn_bins=256) -> dict:
        from farkle_ii_amd.roll_census import RollCensus

        S = len(table)
        gps = S // k
        coords, ss = tournament_game_list(S, k, root_seed, shuffle_begin, shuffle_end)
        rounds = np.full(len(coords), int(max_rounds), dtype=np.int64)
        for o in (overrides if overrides is not None else ()):
            if int(o["root_seed"]) == root_seed and int(o["k_or_order"]) == k and shuffle_begin <= int(o["a"]) < shuffle_end and int(o["b"]) < gps:
                rounds[(int(o["a"]) - shuffle_begin) * gps + int(o["b"])] = int(o["max_rounds"])
        census = RollCensus.zeros(S, turn_bins)
        for r in np.unique(rounds).tolist():
            pick = np.flatnonzero(rounds == r)
            _, begin, events = trace_oracle.pinned(coords[pick], table, ss[pick], k, target_score, r)
            census = census.merge(RollCensus.from_events(events, begin, ss[pick], S, turn_bins))
        return {name: getattr(census, name) for name in CENSUS_TABLES}
