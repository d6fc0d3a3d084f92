"""TEST INFRASTRUCTURE ONLY — ``fk_h2h_round_robin`` restated on the CPU oracle engine (``oracle_engine_stub.Engine``): the pairs are
enumerated with ``itertools.combinations``, every (pair, order) block is played by the stub's ``h2h_blocks`` at ``chunk_games =
max_attempts`` (the oracle's ``h2h_block``), and the summary is built here in NumPy, column by column — none of it through
``farkle_ii_amd.round_robin``, which the tests hold against this.  Also the tables the round-robin tests share."""
from __future__ import annotations

from itertools import combinations

import numpy as np

from oracle_engine_stub import Engine as OracleEngine

HARD = dict(root_seed=11, target=37, max_attempts=74, max_rounds=24)  # the hard case of tests/test_round_robin_gpu.py


def random_valid_table(n: int, seed: int) -> np.ndarray:
    """The recipe of the parity tests' ``_random_valid_table``: random flags under the reference's two validity rules."""
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=STRATEGY_DTYPE)
    t["score_threshold"] = rng.integers(2, 21, n) * 50
    t["dice_threshold"] = rng.integers(0, 5, n)
    for name in ("smart_five", "consider_score", "consider_dice", "auto_hot_dice", "run_up_score", "favor_score"):
        t[name] = rng.integers(0, 2, n)
    t["smart_one"] = t["smart_five"] & rng.integers(0, 2, n).astype(np.uint8)                              # strategies.py:198
    t["require_both"] = t["consider_score"] & t["consider_dice"] & rng.integers(0, 2, n).astype(np.uint8)  # :202
    t["strategy_id"] = np.arange(n)
    return t


def hard_table() -> np.ndarray:
    """Twelve strategies, rows 0 and 1 never bank: their pair never completes a game, and every pair with one of them runs long."""
    t = random_valid_table(12, 3)
    for row in (0, 1):
        t["dice_threshold"][row] = 0
        for name in ("consider_dice", "consider_score", "require_both"):
            t[name][row] = 1
    return t


def enumerate_blocks(table: np.ndarray, pair_begin: int = 0, pair_end: int | None = None):
    """(seats [blocks, 2], pair_ids, orders) of the range in (pair, order) order, by itertools."""
    pairs = list(combinations(range(len(table)), 2))
    end = len(pairs) if pair_end is None else pair_end
    seats, pids, orders = [], [], []
    for pid in range(pair_begin, end):
        i, j = pairs[pid]
        for order in (0, 1):
            seats.append(table[[i, j]] if order == 0 else table[[j, i]])
            pids.append(pid)
            orders.append(order)
    seats = np.stack(seats) if seats else np.zeros((0, 2), dtype=table.dtype)
    return seats, pids, orders


def summary_of(n: int, states: np.ndarray, target: int, pair_begin: int, pair_end: int) -> np.ndarray:
    pairs = list(combinations(range(n), 2))
    out = np.zeros((n, 8), dtype=np.int64)
    st = states.astype(np.int64)
    for row, pid in enumerate(range(pair_begin, pair_end)):
        i, j = pairs[pid]
        a, b = st[row, 0], st[row, 1]
        resolved = int(a[1] >= target and b[1] >= target)
        wins = {i: a[3] + b[4], j: a[4] + b[3]}
        for s, other, first in ((i, j, a), (j, i, b)):  # `first`: the block in which s sits in seat 1
            out[s] += [1, resolved, a[1] + b[1], a[2] + b[2], wins[s], first[1], first[3], int(resolved and wins[s] > wins[other])]
    return out


class Engine(OracleEngine):
    def h2h_round_robin(self, table, root_seed, target, max_attempts, pair_begin=0, pair_end=None, target_score=10_000, max_rounds=200,
                        summary=None):
        table = np.ascontiguousarray(table).reshape(-1)
        n = len(table)
        end = n * (n - 1) // 2 if pair_end is None else int(pair_end)
        if n < 2 or not 0 <= pair_begin <= end <= n * (n - 1) // 2 or not 1 <= target <= max_attempts:
            raise ValueError("bad round-robin arguments")
        seats, pids, orders = enumerate_blocks(table, pair_begin, end)
        flat = self.h2h_blocks(seats, root_seed, pids, orders, target, max_attempts, chunk_games=max_attempts, target_score=target_score,
                               max_rounds=max_rounds) if len(pids) else np.zeros((0, 5), dtype=np.uint64)
        states = flat.reshape(-1, 2, 5).astype(np.uint32)
        if summary is None:
            summary = np.zeros((n, 8), dtype=np.int64)
        summary += summary_of(n, states, target, pair_begin, end)
        return states, summary
