"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine (``oracle_engine_stub.Engine``) plus the two calls of the RNG diagnostics'
matchup family, served from the oracle's ROWS with the host statement of the rule (``farkle_ii_amd.rng_matchups``)."""
from __future__ import annotations

import numpy as np

from oracle_engine_stub import Engine as OracleEngine


class Engine(OracleEngine):
    def tournament_matchups(self, table, k, root_seed, shuffle_begin, shuffle_end, lags, strategy_ids, max_players, shuffles_per_batch=None,
                            target_score=10_000, max_rounds=200, overrides=None) -> dict:
        """``fk_tournament_run_matchups``: the strategy-family outputs of ``tournament_lags`` + the per-game records."""
        from farkle_ii_amd.rng_matchups import records_from_rows

        kw = dict(shuffles_per_batch=shuffles_per_batch, target_score=target_score, max_rounds=max_rounds, overrides=overrides)
        res = self.tournament_lags(table, k, root_seed, shuffle_begin, shuffle_end, lags, **kw)
        rows = self.tournament(table, k, root_seed, shuffle_begin, shuffle_end, want_rows=True, **kw)["rows"]
        ids = np.asarray(strategy_ids, dtype=np.int32)
        if len(ids) != len(table) or len(np.unique(ids)) != len(ids):
            raise ValueError("strategy_ids must hold one unique ID per strategy of the table")
        res["matchups"] = records_from_rows(rows, ids, k, max_players)
        return res

    def matchup_reduce(self, records, k, lags, cap):
        from farkle_ii_amd.rng_matchups import host_reduce

        return host_reduce(records, k, lags, cap)
