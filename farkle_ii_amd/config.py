"""Application configuration for the simulation path.

Mirrors the sections of ``src/farkle/config.py`` this path reads — ``io`` :146-150, ``sim`` :230-289, ``screening``
:172-184, ``batching`` :188-192, ``rng`` :154-158 — with the same YAML overlay semantics (``load_app_config`` :1494,
dotted keys, later overlays win), ``--set section.key=value`` coercion (``apply_dot_overrides`` :1692) and path helpers
(``results_root`` :484-492, ``n_dir`` :858, ``simulation_row_dir`` :862-879, ``checkpoint_path`` :881).  Sections that
only configure the reference's analysis pipeline are accepted and carried opaquely.  Superset: ``--set`` also accepts
list values (``sim.n_players_list=[2]``), which the reference can only take from YAML.
"""
from __future__ import annotations

import ast
from dataclasses import dataclass, field, fields
from pathlib import Path
from typing import Any, Mapping, Sequence

import yaml

_OPAQUE_SECTIONS = {"analysis", "ingest", "combine", "trueskill", "head2head", "hgb", "orchestration", "resources", "profile",
                    "robustness", "artifact_contract", "k_aggregation"}


@dataclass
class IOConfig:
    results_dir_prefix: Path = Path("results")
    analysis_subdir: str = "analysis"


@dataclass
class RNGConfig:
    scheme_version: int = 2
    bit_generator: str = "PCG64DXSM"


@dataclass
class ScreeningConfig:
    resolution_delta: float = 0.03
    interval_confidence: float = 0.95
    practical_delta_by_k: dict | None = None
    delta_across_k: float | None = 0.03
    bootstrap_replicates: int = 2_000
    candidate_contribution_size: int = 75
    controls: list = field(default_factory=list)
    mandatory_diagnostics: list = field(default_factory=list)
    max_shuffles_per_root_k: int | None = None
    projected_games_per_second: float | None = None


@dataclass
class BatchingConfig:
    target_batches: int = 100
    min_shuffles_per_batch: int = 30


@dataclass
class SimConfig:
    n_players_list: list[int] = field(default_factory=lambda: [5])
    seed: int = 0
    seed_list: list[int] | None = None
    expanded_metrics: bool = False
    row_dir: Path | None = None
    metric_chunk_dir: Path | None = None
    sidecars: bool = False  # this engine's option: per-artifact <name>.sidecar.json (sidecars.py; contract version 2)
    all_player_batch_dir: Path | None = None  # this engine's option: all-player batch metrics without rows (all_player.py)
    rng_lag_sums: bool = False  # this engine's option: lag sufficient statistics of the RNG diagnostics' strategy family (rng_lags.py)
    rng_matchup_lags: bool = False  # this engine's option: the RNG diagnostics' matchup family + group selection (rng_matchups.py)
    game_stats: bool = False  # this engine's option: the game-stats stage's per-k tables and rare-event summary without rows (game_stats.py)
    rare_events: bool = False  # with game_stats: the per-game rows of rare_events.parquet / rare_events_details.parquet and the quantile thresholds (rare_events.py)
    seat_analysis: bool = False  # this engine's option: the seat-analysis stage's count tables, seat effects and mirrored pairs without rows (seat_analysis.py)
    performance_bootstrap: bool = False  # this engine's option: the performance stage's batch matrices + joint batch bootstrap (performance_bootstrap.py)
    performance: bool = False  # this engine's option: the performance stage's by-k / across-k estimates and, with performance_bootstrap, the descriptive screening frame (performance.py)
    per_n: dict = field(default_factory=dict)
    n_jobs: int | None = None
    mp_start_method: str | None = None
    desired_sec_per_chunk: int = 10
    ckpt_every_sec: int = 30
    progress_logging: dict = field(default_factory=dict)
    score_thresholds: list[int] | None = None
    dice_thresholds: list[int] | None = None
    smart_five_opts: Sequence[bool] | None = None
    smart_one_opts: Sequence[bool] | None = None
    consider_score_opts: Sequence[bool] = (True, False)
    consider_dice_opts: Sequence[bool] = (True, False)
    auto_hot_dice_opts: Sequence[bool] = (True, False)
    run_up_score_opts: Sequence[bool] = (True, False)
    include_stop_at: bool = False
    include_stop_at_heuristic: bool = False

    def resolve_seed_list(self, expected_len: int) -> list[int]:
        if expected_len < 1:
            raise ValueError("expected_len must be >= 1")
        if self.seed_list is not None:
            if len(self.seed_list) != expected_len:
                raise ValueError(f"sim.seed_list must contain exactly {expected_len} seeds, got {self.seed_list!r}")
            return list(self.seed_list)
        if expected_len == 1:
            return [self.seed]
        raise ValueError(f"sim.seed_list must be set for orchestration requiring {expected_len} seeds")

    def populate_seed_list(self, expected_len: int) -> list[int]:
        seeds = self.resolve_seed_list(expected_len)
        self.seed_list = list(seeds)
        if expected_len in {1, 2}:
            self.seed = seeds[0]
        return seeds


@dataclass(frozen=True)
class Head2HeadInferenceConfig:
    """The ``head2head`` fields the round-robin inference and its power plan read, with the reference's defaults (config.py
    ``Head2HeadConfig``)."""
    family_alpha: float = 0.02
    practical_delta: float = 0.03
    delta_equivalence: float | None = None
    min_candidate_completion_rate: float = 0.99
    target_power: float = 0.80
    seat1_advantage_scenarios: tuple = (0.0, 0.03, 0.06)
    sensitivity_deltas: tuple = (0.03, 0.04)
    allow_single_root: bool = True

    def check_plan(self) -> None:
        """What the power plan demands of its settings, as the reference validates them (config.py:2049-2066; the seat-advantage
        scenarios are not locked to the defaults here, and 0.04 need not be among the sensitivity effects)."""
        if not 0.0 < self.family_alpha < 1.0:
            raise ValueError("head2head.family_alpha must be between 0 and 1")
        if not 0.0 < self.target_power < 1.0:
            raise ValueError("head2head.target_power must be between 0 and 1")
        if not self.practical_delta > 0.0:
            raise ValueError("head2head.practical_delta must be positive")
        deltas = self.sensitivity_deltas
        if len(set(deltas)) != len(deltas) or any(not d > 0.0 for d in deltas) or self.practical_delta not in deltas:
            raise ValueError("head2head.sensitivity_deltas must be unique positive values containing the practical delta")


@dataclass
class AppConfig:
    io: IOConfig = field(default_factory=IOConfig)
    sim: SimConfig = field(default_factory=SimConfig)
    rng: RNGConfig = field(default_factory=RNGConfig)
    screening: ScreeningConfig = field(default_factory=ScreeningConfig)
    batching: BatchingConfig = field(default_factory=BatchingConfig)
    opaque: dict = field(default_factory=dict)  # analysis-only sections, untouched
    # run identities a caller hands in (config.py:472-474 of the reference: private, never part of a configuration digest) — what
    # artifact-contract version 3 signs with (contract_v3.py)
    _code_identity: dict | None = field(default=None, init=False, repr=False, compare=False)
    _run_lineage_sha256: str | None = field(default=None, init=False, repr=False, compare=False)
    _game_profile_sha256: str | None = field(default=None, init=False, repr=False, compare=False)

    @property
    def results_root(self) -> Path:
        base = Path(self.io.results_dir_prefix)
        if not base.is_absolute():
            base = Path("data") / base
        suffix = f"_seed_{self.sim.seed}"
        if base.name.endswith(suffix):
            return base
        return base.parent / f"{base.name}{suffix}"

    def n_dir(self, n: int) -> Path:
        return self.results_root / f"{n}_players"

    @property
    def artifact_contract_version(self) -> int:
        """The contract the sidecar writers follow.  ``artifact_contract.artifact_contract_version`` when the configuration states it
        (the section is carried opaquely; the reference's default is 3, config.py:210); otherwise 3 when the caller supplied the code
        identity version 3 signs with, and the structural version 2 when not."""
        stated = (self.opaque.get("artifact_contract") or {}).get("artifact_contract_version")
        if stated is not None:
            return int(stated)
        return 3 if self._code_identity is not None else 2

    def _per_n_dir(self, raw_value, n: int, what: str) -> Path | None:
        if not raw_value:
            return None
        raw_text = str(raw_value)
        try:
            formatted = raw_text.format(n=n, n_players=n, p=f"{n}p")
        except KeyError as exc:
            raise ValueError(f"unknown simulation {what} placeholder: {exc.args[0]}") from exc
        path = Path(formatted)
        if formatted == raw_text and path.name and not path.name.startswith(f"{n}p"):
            path = path.parent / f"{n}p_{path.name}"
        return path if path.is_absolute() else self.n_dir(n) / path

    def simulation_row_dir(self, n: int) -> Path | None:
        return self._per_n_dir(self.sim.row_dir, n, "row-dir")

    def metric_chunk_dir(self, n: int) -> Path | None:
        return self._per_n_dir(self.sim.metric_chunk_dir, n, "metric-chunk-dir")

    def all_player_batch_dir(self, n: int) -> Path | None:
        return self._per_n_dir(self.sim.all_player_batch_dir, n, "all-player-batch-dir")

    @property
    def head2head(self) -> Head2HeadInferenceConfig:
        """``head2head.family_alpha`` / ``practical_delta`` / ``delta_equivalence`` / ``min_candidate_completion_rate`` and the power
        plan's ``target_power`` / ``seat1_advantage_scenarios`` / ``sensitivity_deltas`` / ``allow_single_root``; the section is carried
        opaquely (its other keys belong to the reference's analysis), these are read from it with the reference's defaults.  What the
        power plan demands of its settings is ``Head2HeadInferenceConfig.check_plan``: a run that is handed its block size does not
        depend on them."""
        section = self.opaque.get("head2head") or {}
        values = {}
        for f in fields(Head2HeadInferenceConfig):
            raw = section.get(f.name, f.default)
            if isinstance(raw, str):  # a --set override of an opaque section arrives as text
                raw = _coerce(raw, f.default if f.name == "allow_single_root" else None)
            if raw is None and f.name == "delta_equivalence":
                values[f.name] = None
                continue
            if f.name == "allow_single_root":
                if not isinstance(raw, bool):
                    raise ValueError("head2head.allow_single_root must be true or false")
                values[f.name] = raw
                continue
            if f.name in ("seat1_advantage_scenarios", "sensitivity_deltas"):
                if not isinstance(raw, (list, tuple)) or not raw or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in raw):
                    raise ValueError(f"head2head.{f.name} must be a list of numbers that is not empty")
                values[f.name] = tuple(float(v) for v in raw)
                continue
            if isinstance(raw, bool) or not isinstance(raw, (int, float)):
                raise ValueError(f"head2head.{f.name} must be a number")
            values[f.name] = float(raw)
        return Head2HeadInferenceConfig(**values)

    def rng_diagnostic_lags(self) -> tuple[int, ...]:
        """``analysis.rng_diagnostic_lags`` (config.py:335, validated like :1933-1939); the analysis section is carried opaquely."""
        raw = (self.opaque.get("analysis") or {}).get("rng_diagnostic_lags", (1,))
        lags = tuple(int(v) for v in raw)
        if not lags or any(v < 1 for v in lags) or tuple(sorted(set(lags))) != lags:
            raise ValueError("analysis.rng_diagnostic_lags must be unique increasing positive integers")
        return lags

    def game_stats_margin_thresholds(self) -> tuple[int, ...]:
        """``analysis.game_stats_margin_thresholds`` (config.py:323, default (500, 1000)): integers, one column pair each."""
        raw = (self.opaque.get("analysis") or {}).get("game_stats_margin_thresholds", (500, 1000))
        if isinstance(raw, (str, bytes)) or not hasattr(raw, "__iter__"):
            raise ValueError("analysis.game_stats_margin_thresholds must be a list of integers")
        values = tuple(raw)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in values):
            raise ValueError("analysis.game_stats_margin_thresholds must be a list of integers")
        return tuple(int(v) for v in values)

    def rare_event_target_score(self) -> int:
        """``analysis.rare_event_target_score`` (config.py:325, default 10 000).  The quantile-resolved rare-event thresholds
        (``rare_event_margin_quantile`` / ``rare_event_target_rate``) need the per-game rows: they are refused here."""
        analysis = self.opaque.get("analysis") or {}
        for key in ("rare_event_margin_quantile", "rare_event_target_rate"):
            if analysis.get(key) is not None:
                raise ValueError(f"analysis.{key} resolves its threshold from per-game rows: --game-stats supports fixed thresholds only")
        value = analysis.get("rare_event_target_score", 10_000)
        if isinstance(value, bool) or not isinstance(value, int) or not -(2 ** 31) <= value < 2 ** 31:
            raise ValueError("analysis.rare_event_target_score must be a 32-bit integer")
        return int(value)

    def rare_event_settings(self) -> dict:
        """What ``--rare-events`` reads beside ``game_stats_margin_thresholds``: ``analysis.rare_event_target_score`` (config.py:325),
        ``rare_event_write_details`` (default off), ``rare_event_margin_quantile`` / ``rare_event_target_rate`` (default ``None``;
        each in (0, 1), the reference's messages).  The quantile keys are served here: :meth:`rare_event_target_score` keeps
        refusing them for ``--game-stats`` alone."""
        analysis = self.opaque.get("analysis") or {}
        target = analysis.get("rare_event_target_score", 10_000)
        if isinstance(target, bool) or not isinstance(target, int) or not -(2 ** 31) <= target < 2 ** 31:
            raise ValueError("analysis.rare_event_target_score must be a 32-bit integer")
        out = {"target_score": int(target), "thresholds": self.game_stats_margin_thresholds(),
               "write_details": bool(analysis.get("rare_event_write_details", False)), "margin_quantile": None, "target_rate": None}
        for key, name in (("rare_event_margin_quantile", "margin_quantile"), ("rare_event_target_rate", "target_rate")):
            value = analysis.get(key)
            if value is None:
                continue
            if isinstance(value, bool) or not isinstance(value, (int, float)):
                raise ValueError(f"analysis.{key} must be a number")
            if not 0.0 < float(value) < 1.0:
                raise ValueError(f"{key} must be between 0 and 1")
            out[name] = float(value)
        if len(out["thresholds"]) > 8:
            raise ValueError("--rare-events carries at most 8 margin thresholds per game (analysis.game_stats_margin_thresholds)")
        return out

    def rare_events_path(self) -> Path:
        return self.results_root / "rare_events.parquet"

    def rare_events_details_path(self) -> Path:
        return self.results_root / "rare_events_details.parquet"

    def metrics_stage_dir(self) -> Path:
        """The reference's metrics stage directory in its default stage layout (config.py:798-802: ``analysis/03_metrics``)."""
        return self.results_root / self.io.analysis_subdir / "03_metrics"

    def performance_batch_matrix_path(self, n: int) -> Path:
        """config.py:981-984: ``by_k/<k>p/performance_batch_matrix.npy``."""
        return self.metrics_stage_dir() / "by_k" / f"{n}p" / "performance_batch_matrix.npy"

    def performance_bootstrap_path(self) -> Path:
        """config.py:1001-1004."""
        return self.metrics_stage_dir() / "across_k" / "performance_bootstrap.parquet"

    def performance_control_contrasts_path(self) -> Path:
        """config.py:1006-1009."""
        return self.metrics_stage_dir() / "across_k" / "performance_control_contrasts.parquet"

    def performance_by_k_path(self, n: int) -> Path:
        """The reference's ``performance_by_k_path`` (config.py:986-989), under this engine's file name."""
        return self.metrics_stage_dir() / "by_k" / f"{n}p" / "performance_by_k.parquet"

    def performance_across_k_path(self) -> Path:
        """The reference's ``performance_across_k_path`` (config.py:991-994), under this engine's file name."""
        return self.metrics_stage_dir() / "across_k" / "performance_across_k.parquet"

    def screening_stage_dir(self) -> Path:
        """The reference's screening stage directory (config.py:841-845) beside the metrics stage."""
        return self.results_root / self.io.analysis_subdir / "04_screening"

    def screening_path(self, filename: str = "descriptive_screening.parquet") -> Path:
        """config.py:1298-1301: ``across_k/descriptive_screening.parquet`` (and ``.json``) of the screening stage."""
        return self.screening_stage_dir() / "across_k" / filename

    def seat_batch_counts_path(self, n: int) -> Path:
        """config.py:1098-1101: ``by_k/<k>p/seat_batch_counts.parquet``."""
        return self.metrics_stage_dir() / "by_k" / f"{n}p" / "seat_batch_counts.parquet"

    def seat_effects_by_k_path(self, n: int) -> Path:
        """config.py:1103-1106."""
        return self.metrics_stage_dir() / "by_k" / f"{n}p" / "seat_effects.parquet"

    def seat_population_by_k_path(self, n: int) -> Path:
        """config.py:1108-1111."""
        return self.metrics_stage_dir() / "by_k" / f"{n}p" / "seat_population_effects.parquet"

    def seat_standardized_across_k_path(self) -> Path:
        """config.py:1113-1116."""
        return self.metrics_stage_dir() / "across_k" / "seat_effects_standardized_across_k.parquet"

    def seat_exposure_mixture_diagnostic_path(self) -> Path:
        """config.py:1118-1121."""
        return self.metrics_stage_dir() / "diagnostics" / "seat_exposure_mixture.parquet"

    def seat_selfplay_diagnostic_path(self) -> Path:
        """config.py:1123-1126."""
        return self.metrics_stage_dir() / "diagnostics" / "seat_selfplay_p1.parquet"

    def seat_mirrored_diagnostic_path(self) -> Path:
        """config.py:1128-1131."""
        return self.metrics_stage_dir() / "diagnostics" / "seat_mirrored_games.parquet"

    def root_stability_settings(self) -> dict:
        """What the two-root stability stage reads beside ``screening``: ``robustness.delta_seed_stability`` (config.py:201, default
        0.03), ``robustness.joint_discrepancy_alpha`` (:202, default 0.05) and ``k_aggregation`` (:222-226, default ``equal-k``); both
        sections are carried opaquely, the reference's defaults apply to what they do not set."""
        robustness = self.opaque.get("robustness") or {}
        aggregation = self.opaque.get("k_aggregation") or {}
        threshold = float(robustness.get("delta_seed_stability", 0.03))
        alpha = float(robustness.get("joint_discrepancy_alpha", 0.05))
        if not threshold > 0.0:
            raise ValueError("robustness.delta_seed_stability must be positive")
        if not 0.0 < alpha < 1.0:
            raise ValueError("robustness.joint_discrepancy_alpha must be in (0, 1)")
        method = str(aggregation.get("method", "equal-k"))
        if method not in ("equal-k", "declared-mapping"):
            raise ValueError("k_aggregation.method must be equal-k or declared-mapping")
        declared = aggregation.get("k_weights")
        return {"delta_seed_stability": threshold, "joint_discrepancy_alpha": alpha, "k_aggregation_method": method,
                "declared_k_weights": None if declared is None else {int(k): float(v) for k, v in dict(declared).items()}}

    def root_stability_diagnostic_settings(self) -> dict:
        """What the stage's eight diagnostic frames read beside ``root_stability_settings``: ``robustness.matched_count_fractions``
        (config.py:203, default ``(0.25, 0.5, 0.75, 1.0)``, validated like :1982-1992), ``resources.stage_batch_bytes["performance"]``
        (:435-446: 16 MiB; a configured mapping without the stage falls back to its ``analysis`` entry, as the reference reads it —
        the budget decides the column chunks and with them the summation order) and ``screening.controls``."""
        robustness = self.opaque.get("robustness") or {}
        raw = robustness.get("matched_count_fractions", (0.25, 0.5, 0.75, 1.0))
        if isinstance(raw, str):  # a --set override of an opaque section arrives as text
            raw = [part for part in raw.replace("[", " ").replace("]", " ").replace(",", " ").split()]
        try:
            fractions = tuple(float(v) for v in raw)
        except (TypeError, ValueError):
            fractions = ()
        if not fractions or any(not 0.0 < f <= 1.0 for f in fractions) or tuple(sorted(set(fractions))) != fractions or fractions[-1] != 1.0:
            raise ValueError("robustness.matched_count_fractions must be unique increasing values in (0, 1] ending at 1")
        budgets = (self.opaque.get("resources") or {}).get("stage_batch_bytes")
        if budgets is None:
            budget = 16 * 1024 * 1024
        else:
            if not isinstance(budgets, dict) or not budgets or any(
                    not isinstance(stage, str) or not stage or isinstance(value, bool) or not isinstance(value, int) or value < 1
                    for stage, value in budgets.items()):
                raise ValueError("resources.stage_batch_bytes must contain positive integer stage budgets")
            if "performance" not in budgets and "analysis" not in budgets:
                raise ValueError("resources.stage_batch_bytes names neither the performance nor the analysis stage")
            budget = int(budgets.get("performance", budgets.get("analysis")))
        return {"matched_count_fractions": fractions, "stage_batch_bytes": budget, "controls": [int(c) for c in self.screening.controls]}

    def game_stats_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_game_stats.parquet"

    def game_stats_sums_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_game_stats_sums.parquet"

    def game_stats_rare_summary_path(self) -> Path:
        return self.results_root / "game_stats_rare_event_summary.parquet"

    def roll_diagnostics_dir(self) -> Path:
        """``diagnostics/`` of the game-stats stage (config.py:949-957), beside this engine's game-stats frames at the results root."""
        return self.results_root / "diagnostics"

    def exact_roll_distribution_path(self) -> Path:
        return self.roll_diagnostics_dir() / "roll_outcome_distribution_exact.parquet"

    def exact_roll_summary_path(self) -> Path:
        return self.roll_diagnostics_dir() / "roll_summary_exact.parquet"

    def observed_roll_distribution_path(self) -> Path:
        return self.roll_diagnostics_dir() / "roll_outcome_distribution_observed.parquet"

    def roll_fit_path(self) -> Path:
        return self.roll_diagnostics_dir() / "roll_fit.parquet"

    def strategy_turns_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_strategy_turns.parquet"

    def rng_max_matchup_groups(self) -> int | None:
        """``analysis.rng_max_matchup_groups`` (config.py:333, validated like :1928-1932): ``None`` or a positive integer."""
        cap = (self.opaque.get("analysis") or {}).get("rng_max_matchup_groups", 100_000)
        if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or cap < 1):
            raise ValueError("analysis.rng_max_matchup_groups must be positive when configured")
        return cap

    def rng_diagnostic_partitions(self) -> int:
        """``analysis.rng_diagnostic_partitions`` (config.py:337, validated like :1940-1947); echoed in the selection report."""
        parts = (self.opaque.get("analysis") or {}).get("rng_diagnostic_partitions", 32)
        if isinstance(parts, bool) or not isinstance(parts, int) or parts < 1 or parts > 256:
            raise ValueError("analysis.rng_diagnostic_partitions must be in [1, 256]")
        return parts

    def combine_max_players(self) -> int:
        """``combine.max_players`` (config.py:356): the number of ``P#_strategy`` columns the matchup key is padded to."""
        mp = (self.opaque.get("combine") or {}).get("max_players", 12)
        if isinstance(mp, bool) or not isinstance(mp, int) or mp < 1:
            raise ValueError("combine.max_players must be a positive integer")
        return mp

    def rng_matchup_groups_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_rng_matchup_groups.parquet"

    def rng_matchup_stats_path(self) -> Path:
        return self.results_root / "rng_matchup_lag_stats.parquet"

    def rng_group_selection_path(self) -> Path:
        return self.results_root / "rng_group_selection.json"

    def rng_lag_sums_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_rng_lag_sums.parquet"

    def rng_lag_stats_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_rng_lag_stats.parquet"

    def checkpoint_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_checkpoint.pkl"

    def metrics_path(self, n: int) -> Path:
        return self.n_dir(n) / f"{n}p_metrics.parquet"

    def strategy_manifest_root_path(self) -> Path:
        return self.results_root / "strategy_manifest.parquet"


def expand_dotted_keys(mapping: Mapping[str, Any]) -> dict[str, Any]:
    out: dict[str, Any] = {}
    for key, value in mapping.items():
        if isinstance(value, Mapping):
            value = expand_dotted_keys(value)
        parts = str(key).split(".")
        cur = out
        for part in parts[:-1]:
            cur = cur.setdefault(part, {})
            if not isinstance(cur, dict):
                raise ValueError(f"dotted key {key!r} collides with a scalar")
        if isinstance(value, dict) and isinstance(cur.get(parts[-1]), dict):
            cur[parts[-1]] = _deep_merge(cur[parts[-1]], value)
        else:
            cur[parts[-1]] = value
    return out


def _deep_merge(base: dict, overlay: Mapping[str, Any]) -> dict:
    out = dict(base)
    for key, value in overlay.items():
        if isinstance(value, Mapping) and isinstance(out.get(key), dict):
            out[key] = _deep_merge(out[key], value)
        else:
            out[key] = value
    return out


def _fill(section_obj, data: Mapping[str, Any], section_name: str) -> None:
    known = {f.name for f in fields(section_obj)}
    for key, value in data.items():
        if key not in known:
            raise ValueError(f"Unknown option {key!r} in config section {section_name!r}")
        if key in {"row_dir", "metric_chunk_dir", "all_player_batch_dir", "results_dir_prefix"} and value is not None:
            value = Path(value)
        setattr(section_obj, key, value)


def load_app_config(*overlays: Path, seed_list_len: int | None = None) -> AppConfig:
    """Merge YAML overlays (later wins) into an :class:`AppConfig`."""
    data: dict[str, Any] = {}
    for path in overlays:
        with Path(path).open("r", encoding="utf-8") as fh:
            # libyaml's loader when the wheel has it: the same document model, a tenth of the time (4 ms of a 30-ms `farkle run`)
            overlay = yaml.load(fh, Loader=getattr(yaml, "CSafeLoader", yaml.SafeLoader)) or {}
        if not isinstance(overlay, Mapping):
            raise TypeError(f"Config file {path} must contain a mapping")
        data = _deep_merge(data, expand_dotted_keys(overlay))
    cfg = AppConfig()
    for name, section in data.items():
        if name in _OPAQUE_SECTIONS:
            cfg.opaque[name] = section
            continue
        if name not in {"io", "sim", "rng", "screening", "batching"}:
            raise ValueError(f"Unknown config section {name!r}")
        if not isinstance(section, Mapping):
            raise TypeError(f"Config section {name!r} must be a mapping")
        _fill(getattr(cfg, name), section, name)
    players = cfg.sim.n_players_list
    if isinstance(players, list):
        norm = []
        for entry in players:
            try:
                value = int(entry)
            except (TypeError, ValueError) as exc:
                raise ValueError(f"invalid n_players_list entry: {entry!r}") from exc
            if value < 2:
                raise ValueError("sim.n_players_list requires concrete player counts >= 2; select cross-k work with "
                                 "canonical scope settings")
            norm.append(value)
        cfg.sim.n_players_list = norm
    if cfg.sim.seed_list is not None:  # sim.seed_list is canonical; seed = seed_list[0] (config.py:1455-1491)
        cfg.sim.seed_list = [int(s) for s in cfg.sim.seed_list]
        if seed_list_len is not None and len(cfg.sim.seed_list) != seed_list_len:
            raise ValueError(f"load_app_config: sim.seed_list must contain exactly {seed_list_len} seeds, "
                             f"got {cfg.sim.seed_list!r}")
        if cfg.sim.seed_list:
            cfg.sim.seed = cfg.sim.seed_list[0]
    if seed_list_len is not None:
        cfg.sim.populate_seed_list(seed_list_len)
    if cfg.rng.scheme_version != 2 or cfg.rng.bit_generator != "PCG64DXSM":
        raise ValueError("this engine implements RNG scheme v2 with PCG64DXSM only")
    return cfg


def _coerce(raw: str, current: Any) -> Any:
    text = raw.strip()
    if text.startswith("[") or text.startswith("{") or text.startswith("("):
        return ast.literal_eval(text)  # superset of the reference: list-valued overrides
    if isinstance(current, bool):
        low = text.lower()
        if low in {"1", "true", "yes", "on"}:
            return True
        if low in {"0", "false", "no", "off"}:
            return False
        raise ValueError(f"Cannot parse boolean value from {raw!r}")
    if isinstance(current, int):
        return int(text)
    if isinstance(current, float):
        return float(text)
    if isinstance(current, Path):
        return Path(text)
    if current is None:
        if text.lower() in {"null", "none"}:
            return None
        for cast in (int, float):
            try:
                return cast(text)
            except ValueError:
                pass
    return text


def apply_dot_overrides(cfg: AppConfig, pairs: Sequence[str]) -> AppConfig:
    """Apply ``section.option=value`` overrides to ``cfg``."""
    for pair in pairs:
        if "=" not in pair:
            raise ValueError(f"Invalid override {pair!r}")
        key, raw = pair.split("=", 1)
        if "." not in key:
            raise ValueError(f"Invalid override {pair!r}")
        section_name, option = key.split(".", 1)
        if section_name in _OPAQUE_SECTIONS:
            cfg.opaque.setdefault(section_name, {})[option] = raw
            continue
        section = getattr(cfg, section_name, None)
        if section is None or section_name == "opaque":
            raise AttributeError(f"Unknown config section {section_name!r}")
        if not hasattr(section, option):
            raise AttributeError(f"Unknown option {option!r} in section {section_name!r}")
        value = _coerce(raw, getattr(section, option))
        if option in {"row_dir", "metric_chunk_dir", "all_player_batch_dir", "results_dir_prefix"} and value is not None:
            value = Path(value)
        setattr(section, option, value)
    return cfg
