"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine (``oracle_engine_stub.Engine``) plus the bootstrap call, served by the NumPy host
statement of the stage (``farkle_ii_amd.performance_bootstrap.host_bootstrap``)."""
from __future__ import annotations

from oracle_engine_stub import Engine as OracleEngine


class Engine(OracleEngine):
    def performance_bootstrap(self, root_seed, ks, wins, exposures, replicate_begin, replicate_end, top_n, delta, controls=(),
                              want_scores=True, contrast_sum=None, contrast_square_sum=None) -> dict:
        """``fk_performance_bootstrap``."""
        from farkle_ii_amd.performance_bootstrap import host_bootstrap

        return host_bootstrap(root_seed, ks, wins, exposures, replicate_begin, replicate_end, top_n, delta, controls=controls,
                              want_scores=want_scores, contrast_sum=contrast_sum, contrast_square_sum=contrast_square_sum)
