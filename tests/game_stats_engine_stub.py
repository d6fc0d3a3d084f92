"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine (``oracle_engine_stub.Engine``) plus the game-stats call, served from the
oracle's ROWS with the host statement of the stage (``farkle_ii_amd.game_stats.GameStatsSummary.from_rows``)."""
from __future__ import annotations

import numpy as np

from oracle_engine_stub import Engine as OracleEngine


class Engine(OracleEngine):
    def tournament_game_stats(self, table, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch=None, target_score=10_000,
                              max_rounds=200, overrides=None, rare_target_score=10_000, want_seat_stats=False, spill_capacity=4096) -> dict:
        """``fk_tournament_run_game_stats``: the tally (+ the all-player arrays) of ``tournament`` and the game statistics."""
        from farkle_ii_amd.game_stats import GameStatsSummary

        kw = dict(shuffles_per_batch=shuffles_per_batch, target_score=target_score, max_rounds=max_rounds, overrides=overrides)
        res = self.tournament(table, k, root_seed, shuffle_begin, shuffle_end, want_rows=True, want_seat_stats=want_seat_stats, **kw)
        ov = np.asarray(overrides["max_rounds"]) if overrides is not None and len(overrides) else np.zeros(0)
        R = max([int(max_rounds)] + [int(v) for v in ov])
        g = GameStatsSummary.from_rows(res["rows"], k, len(table), rare_target_score).to_arrays()
        for name in ("strategy_rounds", "game_rounds"):  # the engine's width: R + 1
            a = g[name]
            g[name] = np.zeros(a.shape[:-1] + (max(R + 1, a.shape[-1]),), np.int64)
            g[name][..., :a.shape[-1]] = a
        g.pop("k")
        return {"tally": res["tally"], "seat_stats": res.get("seat_stats") if want_seat_stats else None,
                "seat_ratio_sums": res.get("seat_ratio_sums") if want_seat_stats else None, "spilled": 0, "game_stats": g}
