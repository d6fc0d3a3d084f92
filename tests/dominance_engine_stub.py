"""TEST INFRASTRUCTURE ONLY — the resident round robin, ``rr_inference`` and ``rr_dominance`` restated on the CPU: the round robin of
``round_robin_engine_stub.Engine`` (the oracle's blocks) keeps its states here instead of on a device, the inference is the host
statement ``rr_inference.infer``, the graphs are the host statement ``dominance.graph`` over its rows."""
from __future__ import annotations

import numpy as np

import round_robin_engine_stub
from farkle_ii_amd import dominance as dom
from farkle_ii_amd import rr_inference as ri


class Engine(round_robin_engine_stub.Engine):
    def rr_counts_reset(self):
        self._rr = None

    def h2h_round_robin_resident(self, table, root_seed, target, max_attempts, pair_begin=0, pair_end=None, target_score=10_000, max_rounds=200,
                                 summary=None, family_pair_count=None):
        states, summary = self.h2h_round_robin(table, root_seed, target, max_attempts, pair_begin, pair_end, target_score, max_rounds, summary)
        if getattr(self, "_rr", None) is None:
            self._rr = {"n": len(table), "begin": int(pair_begin), "states": [], "targets": [], "caps": []}
        self._rr["states"].append(states), self._rr["targets"].append(target), self._rr["caps"].append(max_attempts)
        return summary

    def rr_inference(self, family_alpha=0.02, practical_delta=0.03, delta_equivalence=None, min_candidate_completion_rate=0.99,
                     family_pair_count=None, rows=None, want_strategies=True):
        r = self._rr
        counts = ri.combine_counts(r["states"], r["targets"], r["caps"])
        return ri.infer(r["n"], counts, pair_begin=r["begin"], family_alpha=family_alpha, practical_delta=practical_delta,
                        delta_equivalence=delta_equivalence, min_candidate_completion_rate=min_candidate_completion_rate,
                        family_pair_count=family_pair_count, rows=rows)

    def rr_dominance(self, family_alpha=0.02, practical_delta=0.03, delta_equivalence=None, min_candidate_completion_rate=0.99,
                     family_pair_count=None, rank=None, want_adjacency=True):
        r = self._rr
        if r["begin"] != 0 or len(r["states"][0]) != r["n"] * (r["n"] - 1) // 2:
            raise ValueError("a dominance graph needs the whole family")
        inferred = self.rr_inference(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count)
        rows = inferred["rows"]
        out = dom.graph(r["n"], rows["decision_class"], rows["simultaneous_d_low"], rows["simultaneous_d_high"], rows["balanced_a_win_rate"],
                        practical_delta, rank=rank)
        out["class_counts"] = np.asarray(inferred["class_counts"], dtype=np.int64)
        return out
