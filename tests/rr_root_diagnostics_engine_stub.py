"""TEST INFRASTRUCTURE ONLY — ``dominance_engine_stub.Engine`` (the resident round robin of the oracle's blocks, the inference and the
graphs as host statements) with option ``"rr_keep_roots"`` and ``rr_root_diagnostics`` restated on the CPU: the states the resident
round robin keeps are kept with their root seeds, the diagnostics are the host statement ``rr_root_diagnostics.diagnose``."""
from __future__ import annotations

import dominance_engine_stub
from farkle_ii_amd import rr_root_diagnostics as rd


class Engine(dominance_engine_stub.Engine):
    _keep_roots = 0

    def get_option(self, name):
        if name != "rr_keep_roots":
            raise ValueError(f"unknown option {name}")
        return self._keep_roots

    def set_option(self, name, value):
        if name != "rr_keep_roots":
            return super().set_option(name, value)
        if getattr(self, "_rr", None) is not None:
            raise ValueError("rr_keep_roots cannot change while counts are resident")
        self._keep_roots = int(value)

    def h2h_round_robin_resident(self, table, root_seed, *args, **kwargs):
        kept = getattr(self, "_rr", None)
        if self._keep_roots and kept is not None and int(root_seed) in kept.get("seeds", []):
            raise ValueError(f"root_seed {root_seed} is kept already")
        summary = super().h2h_round_robin_resident(table, root_seed, *args, **kwargs)
        if self._keep_roots:
            self._rr.setdefault("seeds", []).append(int(root_seed))
        return summary

    def rr_root_diagnostics(self, family_alpha=0.02, practical_delta=0.03, delta_equivalence=None, min_candidate_completion_rate=0.99,
                            family_pair_count=None, rows=None, want_agreement=True):
        r = self._rr
        if not r.get("seeds"):
            raise ValueError("no kept roots")
        out = rd.diagnose(r["n"], r["states"], r["seeds"], r["targets"], r["caps"], pair_begin=r["begin"], family_alpha=family_alpha,
                          practical_delta=practical_delta, delta_equivalence=delta_equivalence,
                          min_candidate_completion_rate=min_candidate_completion_rate, family_pair_count=family_pair_count, rows=rows)
        if rows is None:
            out["rows"] = out["agreement"] = None
        elif not want_agreement:
            out["agreement"] = None
        return out
