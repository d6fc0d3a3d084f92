"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine with both bootstrap calls, served by the NumPy host statements of their stages
(``farkle_ii_amd.root_stability.host_root_bootstrap``, ``farkle_ii_amd.performance_bootstrap.host_bootstrap``)."""
from __future__ import annotations

from performance_bootstrap_engine_stub import Engine as BootstrapEngine


class Engine(BootstrapEngine):
    def root_stability_bootstrap(self, roots, ks, wins, exposures, weights, replicate_begin, replicate_end, top_n, observed=None,
                                 expected=None, observed_across=None, expected_across=None, want_membership=False) -> dict:
        """``fk_root_stability_bootstrap``."""
        from farkle_ii_amd.root_stability import host_root_bootstrap

        return host_root_bootstrap(roots, ks, wins, exposures, weights, replicate_begin, replicate_end, top_n, observed=observed,
                                   expected=expected, observed_across=observed_across, expected_across=expected_across,
                                   want_membership=want_membership)
