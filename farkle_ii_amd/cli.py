"""``farkle`` command line for the simulation path: ``run``, ``time``, ``watch``, ``root-stability`` and ``round-robin``.

Mirrors ``src/farkle/cli/main.py`` (:53-140 parser, :325-470 dispatch) for the commands on this path; the
analysis/orchestration commands of the reference are out of scope and are rejected with a clear message.

    python -m farkle_ii_amd --config configs/fast.yaml --set sim.n_players_list=[2] --set sim.seed_list=[42] run --metrics
    python -m farkle_ii_amd time --players 2 --n-games 1000 --seed 42
    python -m farkle_ii_amd watch --seed 42
    python -m farkle_ii_amd --config cfg.yaml watch --players 4 --shuffle 17 --game 3      (replay a tournament game of the config's grid)
    python -m farkle_ii_amd --config cfg.yaml root-stability --root-results data/results_seed_11 --root-results data/results_seed_23
    python -m farkle_ii_amd --config cfg.yaml round-robin --block-games 2191 --strategy-ids family.txt      (every pair, both orders)
    python -m farkle_ii_amd --config cfg.yaml round-robin --plan-power --strategy-ids family.txt      (the block size from the power plan)
    torchrun --nproc-per-node 8 -m farkle_ii_amd --config cfg.yaml run      (one process per GPU, RCCL tally reduce)
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path
from typing import Sequence

LOGGER = logging.getLogger("farkle_ii_amd.cli")
_OUT_OF_SCOPE = ("analyze", "two-seed-pipeline")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="farkle")
    parser.add_argument("--config", type=Path, help="Path to YAML configuration")
    parser.add_argument("--set", dest="overrides", action="append", default=[], metavar="KEY=VALUE",
                        help="Override configuration values")
    parser.add_argument("--log-level", default="INFO", help="Root logging level")
    sub = parser.add_subparsers(dest="command", required=True)
    run = sub.add_parser("run", help="Run a tournament")
    run.add_argument("--metrics", action="store_true", help="Collect per-strategy metrics in addition to win counts")
    run.add_argument("--row-dir", type=Path, help="Write full per-game rows to this directory")
    run.add_argument("--all-player-batches", nargs="?", const=Path("all_player_batches"), type=Path, default=None, metavar="DIR",
                     help="Write the unconditional all-player batch metrics (integer columns of the reference's "
                          "all_player_batch_schema) per deterministic batch, from device accumulators, without rows")
    run.add_argument("--rng-lag-sums", action="store_true",
                     help="Write the lag sufficient statistics of the RNG diagnostics' strategy family (per strategy and "
                          "analysis.rng_diagnostic_lags: pairs, sums, square sums and cross sums of the win indicator and of n_rounds) "
                          "and the autocorrelation rows computed from them, from device accumulators, without rows.  The series spans every "
                          "shuffle of the run and is held in memory until the end: an interrupted --rng-lag-sums run cannot resume (the next "
                          "invocation asks for --force), and a run completed without it must be replayed with --force")
    run.add_argument("--rng-matchup-lags", action="store_true",
                     help="--rng-lag-sums plus the RNG diagnostics' MATCHUP family: per game a digest of the sorted seat tuple and "
                          "n_rounds, grouped on the device; per player count <k>p_rng_matchup_groups.parquet (its top "
                          "analysis.rng_max_matchup_groups eligible groups with their lag sums, counts and histogram), after the last "
                          "player count rng_matchup_lag_stats.parquet and rng_group_selection.json at the results root")
    run.add_argument("--game-stats", action="store_true",
                     help="Write the game-stats stage's tables from device histograms, without rows: per player count "
                          "<k>p_game_stats.parquet (per-strategy and per-k game length, runner-up margin, score spread and close-game "
                          "rates) and <k>p_game_stats_sums.parquet (the exact histograms), after the last player count "
                          "game_stats_rare_event_summary.parquet at the results root (analysis.game_stats_margin_thresholds, "
                          "analysis.rare_event_target_score).  Not resumable: an interrupted run asks for --force")
    run.add_argument("--rare-events", action="store_true",
                     help="With --game-stats: also write rare_events.parquet at the results root (the game rows of every flagged game of "
                          "every player count in the reference's schema and order, then the summary rows) and, with "
                          "analysis.rare_event_write_details, rare_events_details.parquet, from the device's flagged-game list, without "
                          "rows.  Serves analysis.rare_event_margin_quantile / rare_event_target_rate: a histograms-only pass over "
                          "every player count resolves the thresholds, then the same shuffle ranges are replayed to collect the games")
    run.add_argument("--seat-analysis", action="store_true",
                     help="Write the seat-analysis stage's tables from device counts, without rows: per player count "
                          "analysis/03_metrics/by_k/<k>p/seat_batch_counts.parquet, seat_effects.parquet and seat_population_effects.parquet, "
                          "after the last player count across_k/seat_effects_standardized_across_k.parquet (k_aggregation) and "
                          "diagnostics/seat_exposure_mixture.parquet, seat_selfplay_p1.parquet and seat_mirrored_games.parquet (the "
                          "mirrored-game pairs of k = 2).  Runs without rows and the other analysis options.  Not resumable: an interrupted "
                          "run asks for --force")
    run.add_argument("--performance-bootstrap", action="store_true",
                     help="Write the performance stage's joint deterministic-batch bootstrap from the device: per player count "
                          "analysis/03_metrics/by_k/<k>p/performance_batch_matrix.npy (wins / exposures per batch and strategy), after the "
                          "last player count across_k/performance_bootstrap.parquet and across_k/performance_control_contrasts.parquet "
                          "(screening.bootstrap_replicates, delta_across_k, candidate_contribution_size, controls).  May be combined "
                          "with --all-player-batches (the same statistics launch).  Not resumable: an interrupted run asks for --force")
    run.add_argument("--performance", action="store_true",
                     help="Write the performance stage's point estimates from the device: the batch matrices of --performance-bootstrap "
                          "(the same statistics launch) and, after the last player count, per player count "
                          "analysis/03_metrics/by_k/<k>p/performance_by_k.parquet (totals, win rates, Wilson and batch t intervals) and "
                          "across_k/performance_across_k.parquet (equal_k_score, Pareto membership, maximin leader; "
                          "screening.practical_delta_by_k and delta_across_k are required).  With --performance-bootstrap also "
                          "analysis/04_screening/across_k/descriptive_screening.parquet and descriptive_screening.json.  Not "
                          "resumable: an interrupted run asks for --force")
    run.add_argument("--roll-census", nargs="?", const=0, type=int, default=None, metavar="SHUFFLES",
                     help="After the run, census the rolls of the first SHUFFLES shuffles of every player count's range (default: one "
                          "deterministic batch) on the device and hold them against the exact dice law: diagnostics/"
                          "roll_outcome_distribution_exact.parquet and roll_summary_exact.parquet (the reference's exact ordered-roll "
                          "enumeration), roll_outcome_distribution_observed.parquet, roll_fit.parquet (Pearson X^2 per dice count) and per "
                          "player count <k>p_strategy_turns.parquet (farkle rates, points per turn, turn-score quantiles per strategy).  "
                          "Needs no other flag and changes no other artifact of the run.  With several ranks, rank 0 censuses alone "
                          "on its own GPU after the run; the other ranks take no part")
    run.add_argument("--sidecars", action="store_true",
                     help="Write <artifact>.sidecar.json (producer contract + SHA-256 / size of the artifact) beside every output")
    run.add_argument("--code-identity", metavar="COMMIT[:DIRTY_SHA256[:POLICY]]",
                     help="Write artifact-contract-v3 sidecars, sealed shard manifests and the authenticated simulation.done.json, signed with "
                          "this code identity: the one the checkout that will run the reference's `analyze ingest` resolves (its Git commit and, "
                          "for a dirty tree, the worktree fingerprint).  Implies --sidecars")
    run.add_argument("--reference-checkout", type=Path, metavar="PATH",
                     help="Like --code-identity, with the identity resolved from the Git checkout at PATH the way the reference does "
                          "(rev-parse HEAD; staged + worktree diff + inventoried untracked files for a dirty tree)")
    run.add_argument("--force", action="store_true", help="Recompute even when existing run artifacts are available")
    t = sub.add_parser("time", help="Benchmark simulation throughput")
    t.add_argument("--players", type=int, default=5, help="Players per game (default: 5)")
    t.add_argument("--n-games", dest="n_games", type=int, default=1000, help="Number of games to run (default: 1000)")
    t.add_argument("--jobs", type=int, default=1, help="Parallel jobs (accepted for compatibility)")
    t.add_argument("--seed", type=int, default=42, help="Seed (default: 42)")
    w = sub.add_parser("watch", help="Play one game and log every roll, scoring call and decision")
    w.add_argument("--seed", type=int, default=None, help="Seed of the two random strategies and of the game (cli/main.py:103-105)")
    w.add_argument("--config", dest="watch_config", type=Path, default=None, metavar="C",
                   help="Replay a tournament game instead: the root seed and the strategy grid come from this configuration "
                        "(the global --config and --set apply as well)")
    w.add_argument("--players", type=int, default=None, metavar="K", help="Replay: players per game")
    w.add_argument("--shuffle", type=int, default=None, metavar="S", help="Replay: shuffle index of the game's row")
    w.add_argument("--game", type=int, default=None, metavar="G", help="Replay: game index inside the shuffle")
    rs = sub.add_parser("root-stability", help="The two-root stability stage's bootstrap families from two roots' batch matrices")
    rs.add_argument("--root-results", action="append", default=[], type=Path, metavar="DIR",
                    help="Results root of one `farkle run --performance-bootstrap` (its analysis/03_metrics/by_k/<k>p/"
                         "performance_batch_matrix.npy for every player count of sim.n_players_list); exactly two, of different roots")
    rs.add_argument("--out", type=Path, metavar="DIR",
                    help="Write root_bootstrap_top_n_inclusion.parquet, root_discrepancies.parquet and root_joint_discrepancy.parquet under "
                         "DIR/root_stability/ (default: roots_<a>_<b> beside the first results root).  Settings: "
                         "screening.bootstrap_replicates, candidate_contribution_size, practical_delta_by_k, delta_across_k, "
                         "robustness.delta_seed_stability, robustness.joint_discrepancy_alpha, k_aggregation")
    rs.add_argument("--diagnostics", action="store_true",
                    help="Also write the stage's other eight frames beside the three: performance_root_combination_<k>p.parquet per player "
                         "count, performance_root_combination_across_k, root_rank_stability, root_top_n_stability, root_control_movement, "
                         "root_shortlist_changes, root_matched_count_convergence and root_half_drift (further settings: screening.controls, "
                         "robustness.matched_count_fractions, resources.stage_batch_bytes.performance).  All estimates then come from "
                         "one window call on the device")
    rr = sub.add_parser("round-robin", help="Head-to-head round robin: every pair of the strategy table, both seat orders, per root")
    size = rr.add_mutually_exclusive_group(required=True)
    size.add_argument("--block-games", type=int, metavar="N",
                      help="Completed games every (pair, root, order) block must reach; a block plays at most "
                           "ceil(head2head.max_attempt_multiplier x N) attempts (default multiplier 2.0)")
    size.add_argument("--plan-power", action="store_true",
                      help="Size the blocks by the reference's power plan instead: scan the exact power of the score test over every block "
                           "size on the GPU and take the first whose worst seat-advantage scenario reaches head2head.target_power at "
                           "head2head.practical_delta, with the whole table as the family (alpha per pair = family_alpha / pairs) on the "
                           "configured roots.  Writes h2h_power_plan.json and h2h_power_curve.parquet, then runs what --block-games "
                           "<planned> would; with --inference the pair table gains the three plan-derived columns.  Settings: "
                           "head2head.target_power, seat1_advantage_scenarios, sensitivity_deltas, allow_single_root")
    rr.add_argument("--plan-only", action="store_true", help="With --plan-power: stop after the two plan files; no game is played")
    rr.add_argument("--strategy-ids", type=Path, metavar="FILE", help="Restrict the configuration's grid to these strategy ids (one per line)")
    rr.add_argument("--pairs", metavar="BEGIN:END", help="Play this range of pair ids only (default: every pair of the table)")
    rr.add_argument("--blocks", action="store_true", help="Also write round_robin_blocks.parquet: two rows per pair and root")
    rr.add_argument("--out", type=Path, metavar="DIR",
                    help="Write round_robin_pairs.parquet, round_robin_strategies.parquet and round_robin.json under DIR "
                         "(default: <results_root>/h2h_round_robin).  Roots: sim.seed_list")
    rr.add_argument("--inference", action="store_true",
                    help="Keep the block states on the GPU (no round_robin_pairs.parquet), run the score test, the score intervals, Holm's "
                         "adjustment and the decision classes over all roots there, and write round_robin_inference_pairs.parquet, "
                         "round_robin_inference_strategies.parquet and the class counts into round_robin.json.  Settings: "
                         "head2head.family_alpha, practical_delta, delta_equivalence, min_candidate_completion_rate")
    rr.add_argument("--rows", metavar="BEGIN:END",
                    help="With --inference: the pair ids whose rows round_robin_inference_pairs.parquet holds (default: every pair of the "
                         "range when it has at most 2^22 pairs, none beyond)")
    rr.add_argument("--root-diagnostics", action="store_true",
                    help="With --inference on one or two roots: keep every root's states on the GPU too, run the score test, Holm's "
                         "adjustment and the diagnostic decision per root and the agreement between the roots there, and write "
                         "root_pairwise_diagnostics.parquet and root_decision_agreement.parquet (the pairs of --rows) and the "
                         "agreement summary into round_robin.json")
    rr.add_argument("--dominance", action="store_true",
                    help="With --inference over the whole table: build the practical and the statistical dominance graph on the GPU and write "
                         "dominance_edges.parquet (when every pair's row is on the host), cycle_groups.parquet, dominance_fronts.parquet and "
                         "dominance_summary.json")
    rr.add_argument("--screening-scores", type=Path, metavar="FILE",
                    help="With --dominance: a JSON object {strategy id: tournament screening score}, the third key of the display order "
                         "inside a front (default: the column is null)")
    rr.add_argument("--agreement", action="store_true",
                    help="With --inference over the whole table and --candidate-membership: compare the head-to-head decisions with the "
                         "win-rate and the TrueSkill screening rank per pair and count Kendall's pairs of the scored population on the GPU, and "
                         "write agreement_summary.json and (when every pair's row is on the host) selection_conditioned_pairs.parquet")
    rr.add_argument("--candidate-membership", type=Path, metavar="FILE",
                    help="With --agreement: the frozen candidate membership (the reference's candidate_family.parquet) whose final family is "
                         "the strategy table")
    rr.add_argument("--force", action="store_true", help="Replace the tables of an existing output directory")
    for name in _OUT_OF_SCOPE:
        sub.add_parser(name, help="(reference command outside the simulation path)")
    return parser


def _maybe_init_distributed() -> None:
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as dist

        if not dist.is_initialized():
            local = int(os.environ.get("LOCAL_RANK", "0"))
            if torch.cuda.is_available():
                torch.cuda.set_device(local)
                dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            else:
                dist.init_process_group("gloo")


def main(argv: Sequence[str] | None = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.command == "round-robin" and args.plan_only and not args.plan_power:
        parser.error("round-robin: --plan-only belongs to --plan-power")
    logging.basicConfig(level=getattr(logging, str(args.log_level).upper(), logging.INFO),
                        format="%(asctime)s %(levelname)s %(name)s: %(message)s")
    if args.command in _OUT_OF_SCOPE:
        raise SystemExit(f"farkle {args.command}: outside the simulation path this engine replaces; use the reference CLI")
    if args.command == "time":
        from .time_farkle import measure_sim_times

        out = measure_sim_times(n_games=args.n_games, players=args.players, seed=args.seed, jobs=args.jobs)
        print(f"{args.n_games} games, {args.players} players: {out['games_per_sec']:.1f} games/s; winners {out['winners']}")
        return
    replay = args.command == "watch" and (args.watch_config is not None or any(v is not None for v in (args.players, args.shuffle, args.game)))
    if args.command == "watch" and not replay:
        from .watch_game import watch_game

        watch_game(seed=args.seed)  # (no seed: the reference's ValueError)
        return
    from . import runner
    from .config import AppConfig, apply_dot_overrides, load_app_config

    config_path = args.watch_config if replay and args.watch_config is not None else args.config
    cfg = load_app_config(config_path, seed_list_len=None) if config_path is not None else AppConfig()
    cfg = apply_dot_overrides(cfg, list(args.overrides or []))
    if replay:
        from .watch_game import watch_tournament_game

        if args.seed is not None:
            raise SystemExit("farkle watch: --seed plays the reference's two-random-strategy game; a replay takes its root from the configuration")
        if None in (args.players, args.shuffle, args.game):
            raise SystemExit("farkle watch: a replay needs --players, --shuffle and --game")
        if cfg.sim.seed_list is not None and len(cfg.sim.seed_list) != 1:
            raise ValueError(f"sim.seed_list must contain exactly 1 seeds, got {cfg.sim.seed_list!r}")
        cfg.sim.populate_seed_list(1)
        strategies, _ = runner._resolve_strategies(cfg, None)
        watch_tournament_game(strategies, cfg.sim.seed, args.players, args.shuffle, args.game)
        return
    if args.command == "root-stability":
        written = runner.run_root_stability(cfg, args.root_results, out=args.out, diagnostics=args.diagnostics)
        print({name: str(path) for name, path in written.items()})
        return
    if args.command == "round-robin":
        from .h2h_power import PowerPlanError
        from .round_robin import run_round_robin

        try:
            written = run_round_robin(cfg, args.block_games, strategy_ids_file=args.strategy_ids, pairs=args.pairs, blocks=args.blocks,
                                      out=args.out, force=args.force, inference=args.inference, rows=args.rows, dominance=args.dominance,
                                      screening_scores=args.screening_scores, root_diagnostics=args.root_diagnostics, agreement=args.agreement,
                                      candidate_membership=args.candidate_membership, plan_power=args.plan_power, plan_only=args.plan_only)
        except (ValueError, FileExistsError, PowerPlanError) as exc:
            raise SystemExit(f"farkle round-robin: {exc}") from exc
        print({name: str(path) for name, path in written.items()})
        return
    if cfg.sim.seed_list is not None and len(cfg.sim.seed_list) != 1:
        raise ValueError(f"sim.seed_list must contain exactly 1 seeds, got {cfg.sim.seed_list!r}")
    cfg.sim.populate_seed_list(1)
    if args.metrics:
        cfg.sim.expanded_metrics = True
    if args.row_dir is not None:
        cfg.sim.row_dir = args.row_dir
    if args.sidecars:
        cfg.sim.sidecars = True
    if args.code_identity and args.reference_checkout:
        raise SystemExit("farkle run: --code-identity and --reference-checkout are two ways to say the same thing; pass one")
    if args.code_identity or args.reference_checkout:
        from .contract_v3 import parse_code_identity, resolve_code_identity

        cfg._code_identity = parse_code_identity(args.code_identity) if args.code_identity else resolve_code_identity(args.reference_checkout)
        cfg.sim.sidecars = True
    if args.all_player_batches is not None:
        cfg.sim.all_player_batch_dir = args.all_player_batches
    if args.rng_lag_sums:
        cfg.sim.rng_lag_sums = True
    if args.game_stats:
        cfg.sim.game_stats = True
    if args.rare_events:
        if not args.game_stats:
            raise ValueError("--rare-events rides on the game-stats launches: pass --game-stats with it")
        cfg.sim.rare_events = True
    if args.performance_bootstrap:
        cfg.sim.performance_bootstrap = True
    if args.performance:
        cfg.sim.performance = True
    if args.seat_analysis:
        cfg.sim.seat_analysis = True
    if args.rng_matchup_lags:  # (one lag-mode game pass feeds both families)
        cfg.sim.rng_lag_sums = cfg.sim.rng_matchup_lags = True
    _maybe_init_distributed()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("FK_TALLY_REDUCE", "rccl") == "rccl":
        # The per-group tally reduction through the C-ABI's own RCCL communicator (fk_comm_init / fk_reduce_tally): the default
        # whenever it comes up on EVERY rank (the ranks agree on the minimum of their success flags, so none is left on another
        # path); otherwise — and with FK_TALLY_REDUCE=torch — torch.distributed's reduce on the process group.
        from .distributed import agree, init_engine_comm
        from .engine import get_engine

        ok = False
        try:
            ok = bool(init_engine_comm(get_engine()))
        except Exception as exc:  # librccl missing, ncclCommInitRank failed, a CPU-only engine ...
            LOGGER.warning("fk_comm_init failed (%s: %s)", type(exc).__name__, exc)
        everywhere = agree(ok)
        if not everywhere:
            from . import distributed

            distributed._ENGINE_COMM = None
        LOGGER.info("tally reduce: %s", "fk_reduce_tally (RCCL through the C-ABI)" if everywhere else "torch.distributed.reduce")
    rank = int(os.environ.get("RANK", "0"))
    # the resolved configuration beside the results: written on the runner's helper thread, under the first engine call (ctypes drops
    # the GIL for its duration) — 2 ms of a 25-ms `farkle run`; any error of the write surfaces when the run has finished
    active = runner._helper_thread().submit(runner.write_active_config, cfg, cfg.results_root) if rank == 0 else None
    LOGGER.info("Dispatching run command: seed=%s n_players_list=%s results_dir=%s", cfg.sim.seed, cfg.sim.n_players_list,
                cfg.results_root)
    try:
        if len(cfg.sim.n_players_list) > 1 or cfg.sim.performance_bootstrap or cfg.sim.performance or cfg.sim.rare_events:  # (the bootstrap / the rare-event files follow the sweep's last player count)
            out = runner.run_multi(cfg, force=args.force)
        else:
            out = {cfg.sim.n_players_list[0]: runner.run_single_n(cfg, cfg.sim.n_players_list[0], force=args.force)}
    finally:
        if active is not None:
            active.result()
    if args.roll_census is not None:
        runner.run_roll_census(cfg, args.roll_census or None)
    if rank == 0:
        print({f"{k}p_games": v for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1:])
