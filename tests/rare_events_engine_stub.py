"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine plus the rare-events call, served from the oracle's ROWS with the host
statement of the stage (``farkle_ii_amd.rare_events``).  Like the device, a list that does not fit is an ``FK_ERR_ARG`` carrying
the size it needs, and the call is replayed with that room unless ``retry`` is off."""
from __future__ import annotations

import numpy as np

from game_stats_engine_stub import Engine as GameStatsEngine


class Engine(GameStatsEngine):
    calls: list  # (k, shuffle_begin, shuffle_end, rare_target_score, thresholds, want_events) of every rare-events call

    def tournament_rare_events(self, table, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch=None, target_score=10_000,
                               max_rounds=200, overrides=None, rare_target_score=10_000, thresholds=(), want_events=True,
                               want_seat_stats=False, spill_capacity=4096, event_capacity=65_536, retry=True) -> dict:
        from farkle_ii_amd import rare_events as re_
        from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

        if not hasattr(self, "calls"):
            self.calls = []
        self.calls.append((int(k), int(shuffle_begin), int(shuffle_end), int(rare_target_score), tuple(int(t) for t in thresholds),
                           bool(want_events)))
        if not want_events and len(thresholds):
            raise ValueError("the histograms-only call takes no thresholds")
        kw = dict(shuffles_per_batch=shuffles_per_batch, target_score=target_score, max_rounds=max_rounds, overrides=overrides)
        out = self.tournament_game_stats(table, k, root_seed, shuffle_begin, shuffle_end, rare_target_score=rare_target_score,
                                         want_seat_stats=want_seat_stats, **kw)
        rows = self.tournament(table, k, root_seed, shuffle_begin, shuffle_end, want_rows=True, **kw)["rows"]
        s = re_.RareEventSummary.from_rows(rows, k, len(table), rare_target_score)
        head, seats = (re_.events_from_rows(rows, k, len(table) // k, rare_target_score, thresholds) if want_events
                       else (np.zeros((0, 4), np.uint32), np.zeros((0, k), np.uint16)))
        attempts = 1
        if len(head) > int(event_capacity):
            if not retry:
                err = FarkleHipError(FK_ERR_ARG, f"rare events: the event list needs {len(head)} entries, event_capacity is {event_capacity}")
                err.events_needed, err.spill_needed = len(head), 0
                raise err
            attempts = 2
        out.update(attempts=attempts, rare_events={"strategy_second": s.strategy_second, "game_second": s.game_second, "events": len(head),
                                                   "event_head": head, "event_seats": seats})
        return out
