"""TEST INFRASTRUCTURE ONLY — ``rr_root_diagnostics_engine_stub.Engine`` (the resident round robin of the oracle's blocks, the
inference, the graphs and the per-root diagnostics as host statements) with ``agreement_pairs``, ``rr_agreement`` and
``rank_concordance`` restated on the CPU: the host statements of ``farkle_ii_amd.structure_agreement``."""
from __future__ import annotations

import numpy as np

import rr_root_diagnostics_engine_stub
from farkle_ii_amd import structure_agreement as sa


class Engine(rr_root_diagnostics_engine_stub.Engine):
    def agreement_pairs(self, n, decision_class, win_rate_rank, trueskill_rank, want_codes=True):
        codes = sa.pair_codes(n, decision_class, win_rate_rank, trueskill_rank)
        return {"codes": codes if want_codes else None, "counts": sa.pair_counts(codes, decision_class)}

    def rr_agreement(self, win_rate_rank, trueskill_rank, family_alpha=0.02, practical_delta=0.03, delta_equivalence=None,
                     min_candidate_completion_rate=0.99, family_pair_count=None, want_codes=True):
        r = self._rr
        n_pairs = r["n"] * (r["n"] - 1) // 2
        if r["begin"] != 0 or len(r["states"][0]) != n_pairs:
            raise ValueError("pair agreement needs the whole family")
        inferred = self.rr_inference(family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate, family_pair_count, rows=(0, n_pairs))
        out = self.agreement_pairs(r["n"], inferred["rows"]["decision_class"], win_rate_rank, trueskill_rank, want_codes)
        out["class_counts"] = np.asarray(inferred["class_counts"], dtype=np.int64)
        return out

    def rank_concordance(self, x, y):
        if not 2 <= len(x) <= 65536:
            raise ValueError("rank concordance takes 2 to 65536 items")
        return sa.concordance_counts(x, y)
