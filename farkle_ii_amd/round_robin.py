"""Head-to-head round robin: every pair of a strategy table, both seat orders, in one engine call per root.

``Engine.h2h_round_robin`` (``fk_h2h_round_robin``) plays pairs ``[pair_begin, pair_end)`` of a table sorted by strategy id on
the reference's own H2H coordinates and stop rule (``src/farkle/analysis/h2h_schedule.py``: ``_schedule_frame`` :549-606 numbers
the pairs and seats the orders, ``_simulate_block_from_manifest`` :1172-1235 is the prefix rule).  This module is the host side:

* ``pair_count`` / ``unrank`` / ``pair_ids`` — the pair numbering, vectorised (``itertools.combinations(range(n), 2)``);
* ``summary_from_states`` — the host statement of the per-strategy summary the device returns;
* ``blocks_frame`` / ``pairs_frame`` / ``strategies_frame`` — the tables ``farkle round-robin`` writes;
* ``run_round_robin`` — the command: one sequence of engine calls per root of ``sim.seed_list``; with ``--inference`` the states stay
  on the device and the score test, the score intervals, Holm's adjustment and the decision classes of the reference's
  ``h2h_inference.py`` run there (``rr_inference.py`` is their host side); with ``--dominance`` on top, the reference's dominance
  graphs are built there too (``dominance.py`` is their host side); with ``--root-diagnostics`` on top, every root's states are kept
  there as well and the inference per root and the agreement between the roots run there (``rr_root_diagnostics.py``).

Out of scope: the library route of the interval (``confint_proportions_2indep``) is not reproduced; the reference's own complete
inversion is.  Also out of scope: the reference's power plan, schedule hashes, block ids and sidecars;
resuming a partly played round robin; several ranks (pair ranges make the split trivial — a later change).
"""
from __future__ import annotations

import json
import logging
import math
import time
from pathlib import Path
from typing import Any, Sequence

import numpy as np

LOGGER = logging.getLogger(__name__)

STATE_COLS = ("games_attempted", "games_completed", "games_safety_limit", "wins_seat1", "wins_seat2")  # FK_RR_STATE_COLS
SUMMARY_COLS = ("pairs", "pairs_resolved", "games_completed", "games_safety", "wins", "seat1_games_completed", "seat1_wins",
                "pairs_ahead")  # FK_RR_SUMMARY_COLS
BLOCK_SCHEDULE_COLUMNS = ("pair_id", "strategy_a", "strategy_b", "root_seed", "root_index", "order", "order_label", "seat1_strategy",
                          "seat2_strategy", "n_completed_required", "max_attempts")
BLOCK_PROGRESS_COLUMNS = ("games_attempted", "games_completed", "games_safety_limit", "wins_seat1", "wins_seat2", "wins_a", "wins_b",
                          "replacement_attempt_count", "completion_status")
PAIR_COLUMNS = ("pair_id", "strategy_a", "strategy_b", "games_completed", "wins_a", "wins_b", "a_win_rate_order0", "a_win_rate_order1",
                "seat_balanced_a_win_rate", "seat1_win_rate", "resolved")
STRATEGY_COLUMNS = ("strategy_id", *SUMMARY_COLS, "win_rate", "seat1_win_rate")
DEFAULT_MAX_ATTEMPT_MULTIPLIER = 2.0
CALL_BLOCKS = 1 << 22  # blocks one engine call returns at most (80 MB of states): the command walks longer ranges in such calls


def pair_count(n: int) -> int:
    """Pairs of an ``n``-row table."""
    n = int(n)
    if n < 0:
        raise ValueError(f"a table has no negative size, got {n}")
    return n * (n - 1) // 2


def _row_begin(n: int, i):
    i = np.asarray(i, dtype=np.int64)
    return i * (2 * int(n) - i - 1) // 2


def unrank(n: int, pair_id) -> tuple[np.ndarray, np.ndarray]:
    """``pair_id`` -> ``(i, j)``, ``i < j``: the position in ``itertools.combinations(range(n), 2)``.  Closed form in float64 with an
    integer fix-up, as ``rr_unrank`` of the device header."""
    n = int(n)
    pid = np.asarray(pair_id, dtype=np.int64)
    if n < 2:
        raise ValueError(f"a round robin needs at least two strategies, got {n}")
    if pid.size and (int(pid.min()) < 0 or int(pid.max()) >= pair_count(n)):
        raise ValueError(f"pair ids must be in [0, {pair_count(n)}) for {n} strategies")
    b = 2.0 * n - 1.0
    i = ((b - np.sqrt(np.maximum(b * b - 8.0 * pid.astype(np.float64), 0.0))) * 0.5).astype(np.int64)
    i = np.clip(i, 0, n - 2)
    for _ in range(4):  # the closed form is off by one row at most
        i = np.where(_row_begin(n, i) > pid, i - 1, i)
        i = np.where((i < n - 2) & (_row_begin(n, np.minimum(i + 1, n - 1)) <= pid), i + 1, i)
    j = i + 1 + (pid - _row_begin(n, i))
    return i, j


def pair_ids(n: int, pair_begin: int = 0, pair_end: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(pair_id, i, j)`` of the range, in order."""
    begin, end = _check_range(n, pair_begin, pair_end)
    pid = np.arange(begin, end, dtype=np.int64)
    i, j = unrank(n, pid)
    return pid, i, j


def _check_range(n: int, pair_begin: int, pair_end: int | None) -> tuple[int, int]:
    n = int(n)
    if n < 2:
        raise ValueError(f"a round robin needs at least two strategies, got {n}")
    begin, end = int(pair_begin), pair_count(n) if pair_end is None else int(pair_end)
    if begin < 0 or begin > end or end > pair_count(n):
        raise ValueError(f"pair range [{begin}, {end}) is not inside the {pair_count(n)} pairs of {n} strategies")
    return begin, end


def _check_states(n: int, states, pair_begin: int, pair_end: int | None) -> tuple[np.ndarray, int, int]:
    begin, end = _check_range(n, pair_begin, pair_end)
    states = np.asarray(states)
    if states.shape != (end - begin, 2, len(STATE_COLS)):
        raise ValueError(f"states of pair range [{begin}, {end}) must have shape {(end - begin, 2, len(STATE_COLS))}, got {states.shape}")
    return states.astype(np.int64), begin, end


def summary_from_states(n: int, states, target: int, pair_begin: int = 0, pair_end: int | None = None, summary=None) -> np.ndarray:
    """The per-strategy summary of ``fk_h2h_round_robin`` from the block states of a pair range: int64 ``[n, 8]`` (``SUMMARY_COLS``),
    added to ``summary`` when one is given."""
    st, begin, end = _check_states(n, states, pair_begin, pair_end)
    out = np.zeros((int(n), len(SUMMARY_COLS)), dtype=np.int64) if summary is None else summary
    if out.shape != (int(n), len(SUMMARY_COLS)) or out.dtype != np.int64:
        raise ValueError(f"summary must be int64 of shape {(int(n), len(SUMMARY_COLS))}")
    _, i, j = pair_ids(n, begin, end)
    a, b = st[:, 0], st[:, 1]  # order 0: i in seat 1; order 1: j in seat 1
    resolved = ((a[:, 1] >= int(target)) & (b[:, 1] >= int(target))).astype(np.int64)
    wins_i, wins_j = a[:, 3] + b[:, 4], a[:, 4] + b[:, 3]
    ones = np.ones(len(i), dtype=np.int64)
    for idx, cols in ((i, (ones, resolved, a[:, 1] + b[:, 1], a[:, 2] + b[:, 2], wins_i, a[:, 1], a[:, 3], resolved * (wins_i > wins_j))),
                      (j, (ones, resolved, a[:, 1] + b[:, 1], a[:, 2] + b[:, 2], wins_j, b[:, 1], b[:, 3], resolved * (wins_j > wins_i)))):
        for c, values in enumerate(cols):
            np.add.at(out[:, c], idx, values)
    return out


def _ids(strategy_ids, n: int | None = None) -> np.ndarray:
    ids = np.asarray(strategy_ids, dtype=np.int64).reshape(-1)
    if n is not None and len(ids) != n:
        raise ValueError(f"{len(ids)} strategy ids for a table of {n}")
    if len(ids) > 1 and not np.all(ids[1:] > ids[:-1]):
        raise ValueError("strategy ids must be strictly ascending: the pairs are numbered over the table sorted by id")
    return ids


def _roots_states(strategy_ids, roots, states, pair_begin, pair_end) -> tuple[np.ndarray, list[int], list[np.ndarray], int, int]:
    ids = _ids(strategy_ids)
    roots = [int(r) for r in roots]
    states = list(states)
    if not roots or len(roots) != len(states):
        raise ValueError(f"one state array per root: {len(roots)} roots, {len(states)} state arrays")
    checked, begin, end = [], 0, 0
    for st in states:
        arr, begin, end = _check_states(len(ids), st, pair_begin, pair_end)
        checked.append(arr)
    return ids, roots, checked, begin, end


def _status(completed: np.ndarray, attempted: np.ndarray, target: int, max_attempts: int) -> np.ndarray:
    return np.where(completed >= target, "complete", np.where(attempted >= max_attempts, "unresolved_nonviable", "partial_resumable"))


def blocks_frame(strategy_ids, roots: Sequence[int], states: Sequence[np.ndarray], target: int, max_attempts: int, pair_begin: int = 0,
                 pair_end: int | None = None):
    """One row per (pair, root, order), in ``_schedule_frame``'s order: its schedule columns that carry no hash, then the progress
    columns of ``h2h.block_progress``.  ``states[r]`` = the block states of root ``roots[r]`` over the pair range."""
    import pandas as pd

    ids, roots, states, begin, end = _roots_states(strategy_ids, roots, states, pair_begin, pair_end)
    pid, i, j = pair_ids(len(ids), begin, end)
    n_pairs, n_roots = len(pid), len(roots)
    shape = (n_pairs, n_roots, 2)
    st = np.stack(states, axis=1) if n_pairs else np.zeros((0, n_roots, 2, len(STATE_COLS)), dtype=np.int64)  # [pair][root][order][5]
    order = np.broadcast_to(np.arange(2, dtype=np.int64), shape)
    a = np.broadcast_to(ids[i][:, None, None], shape)
    b = np.broadcast_to(ids[j][:, None, None], shape)
    flat = lambda x: np.ascontiguousarray(x).reshape(-1)  # noqa: E731
    attempted, completed, safety, w1, w2 = (flat(st[..., c]) for c in range(len(STATE_COLS)))
    order_f = flat(order)
    frame = pd.DataFrame({
        "pair_id": flat(np.broadcast_to(pid[:, None, None], shape)),
        "strategy_a": flat(a), "strategy_b": flat(b),
        "root_seed": flat(np.broadcast_to(np.asarray(roots, dtype=np.uint64)[None, :, None], shape)),
        "root_index": flat(np.broadcast_to(np.arange(n_roots, dtype=np.int64)[None, :, None], shape)),
        "order": order_f, "order_label": np.where(order_f == 0, "a_b", "b_a"),
        "seat1_strategy": np.where(order_f == 0, flat(a), flat(b)), "seat2_strategy": np.where(order_f == 0, flat(b), flat(a)),
        "n_completed_required": np.full(order_f.shape, int(target), dtype=np.int64),
        "max_attempts": np.full(order_f.shape, int(max_attempts), dtype=np.int64),
        "games_attempted": attempted, "games_completed": completed, "games_safety_limit": safety, "wins_seat1": w1, "wins_seat2": w2,
        "wins_a": np.where(order_f == 0, w1, w2), "wins_b": np.where(order_f == 0, w2, w1),
        "replacement_attempt_count": np.maximum(attempted - int(target), 0),
        "completion_status": _status(completed, attempted, int(target), int(max_attempts)),
    })
    return frame[list(BLOCK_SCHEDULE_COLUMNS + BLOCK_PROGRESS_COLUMNS)]


def _rate(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """``num / den`` in float64, NaN (null in the written tables) where the denominator is 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.full(num.shape, np.nan), where=den > 0)


def pairs_frame(strategy_ids, roots: Sequence[int], states: Sequence[np.ndarray], target: int, pair_begin: int = 0,
                pair_end: int | None = None):
    """One row per pair: the roots pooled within an order, then the equal-order mean of the two orders' rates (the reference's
    ``equal_seat_order_rates`` baseline).  ``resolved``: every block of the pair, over all roots, reached ``target``."""
    import pandas as pd

    ids, roots, states, begin, end = _roots_states(strategy_ids, roots, states, pair_begin, pair_end)
    pid, i, j = pair_ids(len(ids), begin, end)
    pooled = np.sum(states, axis=0) if len(pid) else np.zeros((0, 2, len(STATE_COLS)), dtype=np.int64)  # [pair][order][5]
    a, b = pooled[:, 0], pooled[:, 1]
    rate0, rate1 = _rate(a[:, 3], a[:, 1]), _rate(b[:, 4], b[:, 1])  # a sits in seat 1 in order 0, in seat 2 in order 1
    resolved = np.all([(st[:, :, 1] >= int(target)).all(axis=1) for st in states], axis=0) if len(pid) else np.zeros(0, dtype=bool)
    frame = pd.DataFrame({
        "pair_id": pid, "strategy_a": ids[i], "strategy_b": ids[j], "games_completed": a[:, 1] + b[:, 1], "wins_a": a[:, 3] + b[:, 4],
        "wins_b": a[:, 4] + b[:, 3], "a_win_rate_order0": rate0, "a_win_rate_order1": rate1,
        "seat_balanced_a_win_rate": 0.5 * (rate0 + rate1), "seat1_win_rate": _rate(a[:, 3] + b[:, 3], a[:, 1] + b[:, 1]),
        "resolved": resolved,
    })
    return frame[list(PAIR_COLUMNS)]


def strategies_frame(strategy_ids, summary):
    """One row per strategy: the summary columns, ``win_rate = wins / games_completed`` and ``seat1_win_rate = seat1_wins /
    seat1_games_completed``, null where the denominator is 0."""
    import pandas as pd

    ids = _ids(strategy_ids)
    summary = np.asarray(summary)
    if summary.shape != (len(ids), len(SUMMARY_COLS)):
        raise ValueError(f"summary must have shape {(len(ids), len(SUMMARY_COLS))}, got {summary.shape}")
    summary = summary.astype(np.int64)
    data: dict[str, Any] = {"strategy_id": ids}
    data.update({name: summary[:, c] for c, name in enumerate(SUMMARY_COLS)})
    data["win_rate"] = _rate(summary[:, 4], summary[:, 2])
    data["seat1_win_rate"] = _rate(summary[:, 6], summary[:, 5])
    return pd.DataFrame(data)[list(STRATEGY_COLUMNS)]


def max_attempts_for(block_games: int, multiplier: float = DEFAULT_MAX_ATTEMPT_MULTIPLIER) -> int:
    """``ceil(multiplier x block_games)`` (``_schedule_frame``, h2h_schedule.py:563); the multiplier is refused unless finite and at
    least 1 (the reference's config.py:2079)."""
    multiplier = float(multiplier)
    if not math.isfinite(multiplier) or multiplier < 1.0:
        raise ValueError("head2head.max_attempt_multiplier must be finite and at least 1")
    if int(block_games) < 1:
        raise ValueError(f"--block-games must be at least 1, got {block_games}")
    return math.ceil(multiplier * int(block_games))


def read_strategy_ids(path) -> list[int]:
    """One strategy id per line (blank lines skipped)."""
    out = []
    for line_no, line in enumerate(Path(path).read_text().splitlines(), 1):
        text = line.strip()
        if not text:
            continue
        if not text.isdigit():
            raise ValueError(f"{path}:{line_no}: not a strategy id: {text!r}")
        out.append(int(text))
    return out


def select_strategies(strategies, wanted_ids: Sequence[int] | None):
    """The grid restricted to ``wanted_ids`` (all of it when none are given), sorted by strategy id."""
    by_id = {int(s.strategy_id): s for s in strategies}
    if len(by_id) != len(strategies):
        raise ValueError("round-robin: the strategy grid carries duplicate strategy ids")
    if wanted_ids is not None:
        wanted = [int(v) for v in wanted_ids]
        dup = sorted({v for v in wanted if wanted.count(v) > 1}) if len(set(wanted)) != len(wanted) else []
        if dup:
            raise ValueError(f"round-robin: duplicate strategy ids in the id file: {dup[:10]}")
        missing = sorted(v for v in wanted if v not in by_id)
        if missing:
            raise ValueError(f"round-robin: strategy ids not in the configuration's grid: {missing[:10]}")
        by_id = {v: by_id[v] for v in wanted}
    chosen = [by_id[v] for v in sorted(by_id)]
    if len(chosen) < 2:
        raise ValueError(f"round-robin: a round robin needs at least two strategies, got {len(chosen)}")
    return chosen


def parse_pair_range(text: str | None, n: int) -> tuple[int, int]:
    """``BEGIN:END`` (either side may be empty) inside the pairs of ``n`` strategies."""
    if text is None:
        return 0, pair_count(n)
    parts = str(text).split(":")
    if len(parts) != 2 or any(p and not p.isdigit() for p in parts):
        raise ValueError(f"round-robin: --pairs takes BEGIN:END, got {text!r}")
    begin = int(parts[0]) if parts[0] else 0
    end = int(parts[1]) if parts[1] else pair_count(n)
    if begin > end or end > pair_count(n):
        raise ValueError(f"round-robin: pair range [{begin}, {end}) is not inside the {pair_count(n)} pairs of {n} strategies")
    return begin, end


def run_round_robin(cfg, block_games: int | None, *, strategy_ids_file=None, pairs: str | None = None, blocks: bool = False, out=None,
                    force: bool = False, strategies=None, engine=None, world: int | None = None, inference: bool = False,
                    rows: str | None = None, dominance: bool = False, screening_scores=None, root_diagnostics: bool = False,
                    agreement: bool = False, candidate_membership=None, plan_power: bool = False, plan_only: bool = False) -> dict:
    """``farkle round-robin``: the grid of ``cfg`` (restricted to the ids of ``strategy_ids_file``), every pair of the range, per root of
    ``sim.seed_list``.  Writes ``round_robin_pairs.parquet``, ``round_robin_strategies.parquet``, ``round_robin.json`` and, with
    ``blocks``, ``round_robin_blocks.parquet`` under ``out`` (default ``<results_root>/h2h_round_robin``).  Returns the written paths.

    With ``inference`` the block states stay on the device (``Engine.h2h_round_robin_resident``, one call per root), the inference runs
    once over all roots (``Engine.rr_inference`` with the ``head2head`` settings of ``cfg``) and the command writes
    ``round_robin_inference_pairs.parquet`` (the pairs of ``rows``, ``BEGIN:END`` in pair ids; default every pair of a range of at most
    2^22 pairs, none beyond), ``round_robin_inference_strategies.parquet``, ``round_robin_strategies.parquet`` and the class counts in
    ``round_robin.json``; the tables that need the states on the host (``round_robin_pairs.parquet``, ``blocks``) are not written.

    With ``dominance`` (and ``inference``, over the whole table) the inference feeds the dominance graphs on the device
    (``Engine.rr_dominance``) and the command also writes the reference's ``cycle_groups.parquet``, ``dominance_fronts.parquet``,
    ``dominance_summary.json`` and — when every pair's row is on the host — ``dominance_edges.parquet`` (``dominance.py`` builds the
    frames; ``round_robin.json`` says when the edges are omitted).  ``screening_scores``: a JSON file ``{strategy id: score}``.

    With ``root_diagnostics`` (and ``inference``, on one or two distinct roots) the engine's option ``"rr_keep_roots"`` is on for the
    run, ``Engine.rr_root_diagnostics`` follows the inference and the command also writes the reference's
    ``root_pairwise_diagnostics.parquet`` and ``root_decision_agreement.parquet`` (the pairs of ``rows``) and the summary under
    ``"root_diagnostics"`` in ``round_robin.json`` (``rr_root_diagnostics.py`` builds the frames).

    With ``agreement`` (and ``inference``, over the whole table) and ``candidate_membership`` — the reference's
    ``candidate_family.parquet``, whose final family is the table — the inference's classes are compared with the two screening ranks on
    the device (``Engine.rr_agreement``), Kendall's pair counts of the scored population are taken there (``Engine.rank_concordance``) and
    the command also writes the reference's ``agreement_summary.json`` and — when every pair's row is on the host —
    ``selection_conditioned_pairs.parquet`` (``structure_agreement.py`` builds both), and the counts under ``"agreement"`` in
    ``round_robin.json``.  ``execution_scope`` is ``root_pair`` on two roots and ``single_root`` on one.

    With ``plan_power`` (and ``block_games`` None) the command sizes its own blocks first: the reference's power plan for the whole table
    as the family, on the configured roots, from the ``head2head`` settings (``h2h_power.plan_from_config``: the device scans the exact
    power of every block size, ``Engine.score_power_scan``).  It writes ``h2h_power_plan.json`` and ``h2h_power_curve.parquet`` under
    ``out`` and then runs what ``block_games`` = the planned size would; ``round_robin.json`` gains ``"power_plan"`` and, with
    ``inference``, the pair table gains the reference's three plan-derived columns.  ``plan_only`` stops after the two files: no game is
    played and no strategy table reaches the device."""
    import os

    import pyarrow as pa

    from . import runner
    from .engine import get_engine
    from .strategies import pack_strategies

    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else int(world)
    if world > 1:
        raise ValueError(f"round-robin: runs on one rank, got a world of {world} (split the work with --pairs; several ranks are a later change)")
    multiplier = cfg.opaque.get("head2head", {}).get("max_attempt_multiplier", DEFAULT_MAX_ATTEMPT_MULTIPLIER)
    if plan_power == (block_games is not None):
        raise ValueError("round-robin: exactly one of --block-games and --plan-power sizes the blocks")
    if plan_only and not plan_power:
        raise ValueError("round-robin: --plan-only belongs to --plan-power")
    max_attempts = max_attempts_for(1 if plan_power else block_games, multiplier)  # (a plan: the multiplier's check; the cap follows the plan)
    target = 0 if plan_power else int(block_games)
    if strategies is None:
        strategies, _ = runner._resolve_strategies(cfg, None)
    wanted = read_strategy_ids(strategy_ids_file) if strategy_ids_file is not None else None
    chosen = select_strategies(strategies, wanted)
    ids = [int(s.strategy_id) for s in chosen]
    n = len(chosen)
    begin, end = parse_pair_range(pairs, n)
    if inference:
        if blocks:
            raise ValueError("round-robin: --blocks needs the block states on the host, --inference keeps them on the GPU: choose one")
        if begin == end:
            raise ValueError("round-robin: --inference needs a pair range that is not empty")
        from . import rr_inference as ri

        h2h = cfg.head2head
        family = pair_count(n)  # the reference's unordered_pair_count: the family is the table's, whatever range this run plays
        ri.check_params(end - begin, h2h.family_alpha, h2h.practical_delta, h2h.delta_equivalence, h2h.min_candidate_completion_rate, family)
        if rows is None:
            row_range = (begin, end) if end - begin <= ri.DEFAULT_ROWS_LIMIT else (begin, begin)
        else:
            parts = str(rows).split(":")
            ok = len(parts) == 2 and all(not p or p.isdigit() for p in parts)
            row_range = (int(parts[0]) if parts[0] else begin, int(parts[1]) if parts[1] else end) if ok else (0, 0)
            if not ok or not begin <= row_range[0] <= row_range[1] <= end:
                raise ValueError(f"round-robin: --rows takes BEGIN:END inside the played pair range [{begin}, {end}), got {rows!r}")
    elif rows is not None:
        raise ValueError("round-robin: --rows belongs to --inference")
    scores = None
    if dominance:
        from . import dominance as dom

        if not inference:
            raise ValueError("round-robin: --dominance belongs to --inference")
        if (begin, end) != (0, pair_count(n)):
            raise ValueError(f"round-robin: --dominance needs every pair of the table, --pairs plays [{begin}, {end}) of {pair_count(n)}")
        if n > dom.DOM_MAX_N:
            raise ValueError(f"round-robin: --dominance holds at most {dom.DOM_MAX_N} strategies, got {n}")
        if screening_scores is not None:
            scores = {int(k): float(v) for k, v in json.loads(Path(screening_scores).read_text()).items()}
            missing = sorted(set(ids) - set(scores))
            if missing:
                raise ValueError(f"round-robin: {screening_scores} lacks the screening scores of strategies {missing[:10]}")
    elif screening_scores is not None:
        raise ValueError("round-robin: --screening-scores belongs to --dominance")
    roots = [int(r) for r in (cfg.sim.seed_list if cfg.sim.seed_list else [cfg.sim.seed])]
    if root_diagnostics:
        from . import rr_root_diagnostics as rd

        if not inference:
            raise ValueError("round-robin: --root-diagnostics belongs to --inference")
        try:
            rd.check_roots(roots)
        except ValueError as exc:
            raise ValueError(f"round-robin: --root-diagnostics: {exc}") from exc
    if agreement:
        from . import structure_agreement as sa

        if not inference:
            raise ValueError("round-robin: --agreement belongs to --inference")
        if candidate_membership is None:
            raise ValueError("round-robin: --agreement needs --candidate-membership")
        if (begin, end) != (0, pair_count(n)):
            raise ValueError(f"round-robin: --agreement needs every pair of the table, --pairs plays [{begin}, {end}) of {pair_count(n)}")
        if len(roots) not in sa.EXECUTION_SCOPES:
            raise ValueError(f"round-robin: --agreement runs on one or two roots, got {len(roots)}")
        try:
            membership = sa.read_membership(candidate_membership, ids)
        except ValueError as exc:
            raise ValueError(f"round-robin: --candidate-membership {candidate_membership}: {exc}") from exc
    elif candidate_membership is not None:
        raise ValueError("round-robin: --candidate-membership belongs to --agreement")
    out_dir = Path(out) if out is not None else cfg.results_root / "h2h_round_robin"
    if out_dir.exists() and not force:
        raise FileExistsError(f"round-robin: {out_dir} exists; pass --force to replace its tables")
    eng = engine or get_engine()
    written_plan: dict = {}
    if plan_power:
        from . import h2h_power as hp

        planned = hp.plan_from_config(eng, cfg.head2head, n, roots)
        plan_doc = hp.plan_document(planned, cfg.head2head, multiplier)
        out_dir.mkdir(parents=True, exist_ok=True)
        written_plan = {"power_plan": out_dir / "h2h_power_plan.json", "power_curve": out_dir / "h2h_power_curve.parquet"}
        runner._atomic_write_bytes(written_plan["power_plan"], (json.dumps(plan_doc, indent=2, sort_keys=True) + "\n").encode("utf-8"))
        runner._write_parquet_atomic(pa.Table.from_pandas(hp.curve_frame(planned), preserve_index=False), written_plan["power_curve"])
        LOGGER.info("round robin power plan: %d games per (pair, root, order) block, worst-scenario power %.6f (%d sizes scanned)",
                    planned["block_games"], planned["worst_scenario_achieved_power"], len(planned["curve"]))
        if plan_only:
            return written_plan
        target = int(planned["block_games"])
        max_attempts = max_attempts_for(target, multiplier)
    table = pack_strategies(chosen)
    summary = np.zeros((n, len(SUMMARY_COLS)), dtype=np.int64)
    states: list[np.ndarray] = []
    started = time.perf_counter()
    for root in roots if not inference else ():
        parts = []
        for lo in range(begin, end, CALL_BLOCKS // 2):
            st, _ = eng.h2h_round_robin(table, root, target, max_attempts, pair_begin=lo, pair_end=min(end, lo + CALL_BLOCKS // 2), summary=summary)
            parts.append(st)
        states.append(np.concatenate(parts) if parts else np.zeros((0, 2, len(STATE_COLS)), dtype=np.uint32))
        LOGGER.info("round robin root %d: %d pairs, %d attempts", root, end - begin, int(states[-1][:, :, 0].sum(dtype=np.int64)))
    if inference:
        eng.rr_counts_reset()
        keep_before = eng.get_option("rr_keep_roots") if root_diagnostics else 0
        if root_diagnostics:
            eng.set_option("rr_keep_roots", 1)
        try:
            for root in roots:
                eng.h2h_round_robin_resident(table, root, target, max_attempts, pair_begin=begin, pair_end=end, summary=summary,
                                             family_pair_count=family)
                LOGGER.info("round robin root %d: %d pairs, resident", root, end - begin)
            knobs = dict(family_alpha=h2h.family_alpha, practical_delta=h2h.practical_delta, delta_equivalence=h2h.delta_equivalence,
                         min_candidate_completion_rate=h2h.min_candidate_completion_rate)
            result = eng.rr_inference(family_pair_count=family, rows=row_range, **knobs)
            if root_diagnostics:
                diagnosed = eng.rr_root_diagnostics(family_pair_count=family, rows=row_range, **knobs)
            if dominance:
                graphs = eng.rr_dominance(family_pair_count=family, rank=dom.rank_of_ids(ids), **knobs)
            if agreement:
                pairs_written = row_range == (begin, end)  # the frame names every pair's class: its row is on the host
                agreed = eng.rr_agreement(membership["win_rate_rank"], membership["trueskill_rank"], family_pair_count=family,
                                          want_codes=pairs_written, **knobs)
                scored = sa.scored_population(membership)
                concordance = eng.rank_concordance(*scored) if len(scored[0]) >= 2 else None
        finally:
            eng.rr_counts_reset()
            if root_diagnostics:
                eng.set_option("rr_keep_roots", keep_before)
    elapsed = time.perf_counter() - started
    out_dir.mkdir(parents=True, exist_ok=True)
    written = {"strategies": out_dir / "round_robin_strategies.parquet", "json": out_dir / "round_robin.json", **written_plan}
    frames = [(strategies_frame(ids, summary), written["strategies"])]
    if inference:
        written["inference_pairs"] = out_dir / "round_robin_inference_pairs.parquet"
        written["inference_strategies"] = out_dir / "round_robin_inference_strategies.parquet"
        inference_pairs = ri.pairs_frame(result["rows"], ids, family_pair_count=family, **knobs)
        if plan_power:
            inference_pairs = ri.with_plan_columns(inference_pairs, h2h.target_power, planned["worst_scenario_achieved_power"])
        frames.append((inference_pairs, written["inference_pairs"]))
        frames.append((ri.strategies_frame(result["strategies"], ids, h2h.min_candidate_completion_rate), written["inference_strategies"]))
        if root_diagnostics:
            written["root_pairs"] = out_dir / "root_pairwise_diagnostics.parquet"
            written["root_agreement"] = out_dir / "root_decision_agreement.parquet"
            kept = [int(r) for r in diagnosed["roots"]]
            frames.append((rd.root_pairs_frame(diagnosed["rows"], kept, ids, family_alpha=h2h.family_alpha), written["root_pairs"]))
            frames.append((rd.agreement_frame(diagnosed["agreement"], kept, ids), written["root_agreement"]))
        if dominance:
            written["dominance_cycles"] = out_dir / "cycle_groups.parquet"
            written["dominance_fronts"] = out_dir / "dominance_fronts.parquet"
            written["dominance_summary"] = out_dir / "dominance_summary.json"
            frames.append((dom.cycles_frame(graphs["nodes"], graphs["extremes"], graphs["adjacency"], ids), written["dominance_cycles"]))
            frames.append((dom.fronts_frame(graphs["nodes"], result["strategies"], ids, scores), written["dominance_fronts"]))
            edges_written = row_range == (begin, end)
            if edges_written:
                written["dominance_edges"] = out_dir / "dominance_edges.parquet"
                frames.append((dom.edges_frame(result["rows"], ids, h2h.practical_delta), written["dominance_edges"]))
            digest = dom.summary(graphs["nodes"], result["strategies"], graphs["class_counts"], ids)
            runner._atomic_write_bytes(written["dominance_summary"], (json.dumps(digest, indent=2, sort_keys=True) + "\n").encode("utf-8"))
        if agreement:
            written["agreement_summary"] = out_dir / "agreement_summary.json"
            if pairs_written:
                written["agreement_pairs"] = out_dir / "selection_conditioned_pairs.parquet"
                frames.append((sa.pairs_frame(agreed["codes"], result["rows"]["decision_class"], ids, membership["family_hash"]),
                               written["agreement_pairs"]))
            stability = rd.stability_summary(diagnosed["summary"]) if root_diagnostics else None
            agreement_digest = sa.summary(membership, agreed["counts"], concordance, stability, sa.EXECUTION_SCOPES[len(roots)])
            runner._atomic_write_bytes(written["agreement_summary"], (json.dumps(agreement_digest, indent=2, sort_keys=True) + "\n").encode("utf-8"))
    else:
        written["pairs"] = out_dir / "round_robin_pairs.parquet"
        frames.append((pairs_frame(ids, roots, states, target, begin, end), written["pairs"]))
    if blocks:
        written["blocks"] = out_dir / "round_robin_blocks.parquet"
        frames.append((blocks_frame(ids, roots, states, target, max_attempts, begin, end), written["blocks"]))
    for frame, path in frames:
        runner._write_parquet_atomic(pa.Table.from_pandas(frame, preserve_index=False), path)
    if inference:  # every game of a pair is incident to its two strategies
        attempted, completed = int(result["strategies"][:, 7].sum()) // 2, int(result["strategies"][:, 8].sum()) // 2
    else:
        attempted = int(sum(int(st[:, :, 0].sum(dtype=np.int64)) for st in states))
        completed = int(sum(int(st[:, :, 1].sum(dtype=np.int64)) for st in states))
    report = {"strategies": n, "strategy_ids_file": None if strategy_ids_file is None else str(strategy_ids_file), "roots": roots,
              "block_games": target, "max_attempt_multiplier": float(multiplier), "max_attempts": max_attempts,
              "target_score": 10_000, "max_rounds": 200, "pair_begin": begin, "pair_end": end, "pairs_total": pair_count(n),
              "blocks": 2 * (end - begin) * len(roots), "games_attempted": attempted, "games_completed": completed,
              "elapsed_seconds": elapsed, "files": sorted(p.name for p in written.values())}
    if plan_power:
        report["power_plan"] = {key: plan_doc[key] for key in ("n_completed_required_per_root_order_block", "target_power", "target_effect", "alpha_per_pair",
                                                                 "worst_scenario_achieved_power", "previous_equal_block_size_worst_power")}
        report["power_plan"].update(block_sizes_scanned=int(len(planned["curve"])), host_evaluations=int(planned["host_evaluations"]))
    if inference:
        report["inference"] = {"class_counts": {name: int(v) for name, v in zip(ri.DECISION_CLASSES, result["class_counts"])},
                               "family_pair_count": family, "row_begin": row_range[0], "row_end": row_range[1], **knobs}
    if root_diagnostics:
        largest = diagnosed["max_abs_discrepancy"]
        report["root_diagnostics"] = {"roots": kept, "row_begin": row_range[0], "row_end": row_range[1],
                                      "summary": {name: int(v) for name, v in zip(rd.SUMMARY_COLS, diagnosed["summary"])},
                                      "max_abs_discrepancy": None if math.isnan(largest) else float(largest),
                                      "root_specific_h2h_stability": rd.stability_summary(diagnosed["summary"])}
    if dominance:
        report["dominance"] = {"edges_written": edges_written, "screening_scores": None if screening_scores is None else str(screening_scores),
                               **{key: digest[key] for key in ("practical_front_count", "statistical_front_count", "practical_cycle_group_count",
                                                               "statistical_cycle_group_count", "unique_best")}}
        if not edges_written:
            report["dominance"]["edges_omitted"] = "dominance_edges.parquet needs the row of every pair on the host (--rows)"
    if agreement:
        report["agreement"] = {"candidate_membership": str(candidate_membership), "family_hash": membership["family_hash"],
                               "execution_scope": sa.EXECUTION_SCOPES[len(roots)], "pairs_written": pairs_written,
                               "scored_population": int(len(scored[0])),
                               "counts": {name: int(v) for name, v in zip(sa.COUNT_NAMES, agreed["counts"])},
                               "concordance": None if concordance is None else {name: int(v) for name, v in zip(sa.CONCORDANCE_NAMES, concordance)}}
        if not pairs_written:
            report["agreement"]["pairs_omitted"] = "selection_conditioned_pairs.parquet needs the row of every pair on the host (--rows)"
    runner._atomic_write_bytes(written["json"], (json.dumps(report, indent=2, sort_keys=True) + "\n").encode("utf-8"))
    return written
