"""TEST INFRASTRUCTURE ONLY — an ``Engine.trace_games`` stand-in on the CPU oracle (tests/trace_oracle.py), so that what sits on top
of the device trace — ``farkle watch``, ``trace_tournament_game``, ``rows_from_events`` — runs on GPU-less hosts.  Install it with
``farkle_ii_amd.engine.set_engine(TraceEngineStub())``; nothing in the product imports it."""
from __future__ import annotations

import trace_oracle


class TraceEngineStub:
    def __init__(self):
        self.calls = 0

    def trace_games(self, coords, table, seat_strategy, k, target_score=10_000, max_rounds=200):
        self.calls += 1
        return trace_oracle.pinned(coords, table, seat_strategy, k, target_score, max_rounds)
