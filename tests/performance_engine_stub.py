"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine with the bootstrap call (``performance_bootstrap_engine_stub.Engine``) plus the two
point-estimate calls, served by the NumPy host statement of the stage (``farkle_ii_amd.performance.host_by_k`` / ``host_across_k``)."""
from __future__ import annotations

from performance_bootstrap_engine_stub import Engine as BootstrapEngine


class Engine(BootstrapEngine):
    def performance_by_k(self, k, wins, exposures, completed, safety) -> dict:
        """``fk_performance_by_k``."""
        from farkle_ii_amd.performance import host_by_k

        return host_by_k(k, wins, exposures, completed, safety)

    def performance_across_k(self, deltas, variances) -> dict:
        """``fk_performance_across_k``."""
        from farkle_ii_amd.performance import host_across_k

        return host_across_k(deltas, variances)
