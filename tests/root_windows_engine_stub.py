"""TEST INFRASTRUCTURE ONLY — the CPU oracle engine of the two-root stability stage with the window call and Kendall's pair counts,
served by the NumPy host statements ``farkle_ii_amd.root_stability.estimate_windows`` and
``farkle_ii_amd.structure_agreement.concordance_counts``."""
from __future__ import annotations

from root_stability_engine_stub import Engine as RootStabilityEngine


class Engine(RootStabilityEngine):
    def root_window_estimates(self, wins, exposures, completed, safety, windows) -> dict:
        """``fk_root_window_estimates``."""
        from farkle_ii_amd.root_stability import estimate_windows

        return estimate_windows(wins, exposures, completed, safety, windows)

    def rank_concordance(self, x, y):
        """``fk_rank_concordance``."""
        from farkle_ii_amd.structure_agreement import concordance_counts

        if not 2 <= len(x) <= 65536:
            raise ValueError("rank concordance takes 2 to 65536 items")
        return concordance_counts(x, y)
