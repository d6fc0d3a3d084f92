"""TEST INFRASTRUCTURE ONLY — tables and game lists the roll-census tests share (CPU and GPU)."""
from __future__ import annotations

import golden_util as gu
import numpy as np

from farkle_ii_amd.backend import make_coords
from farkle_ii_amd.strategies import STRATEGY_DTYPE


def g64() -> np.ndarray:
    return gu.strategies_from_tuples(gu.load("grid_vectors.json")["g64"], STRATEGY_DTYPE)


def mixed_table() -> np.ndarray:
    """Config 2's 64-strategy grid (every strategy with auto_hot_dice and run_up_score) + sixteen of its strategies with one or both
    flags cleared and the smart discards varied (the table of tests/test_trace_gpu.py): every flag differs somewhere in a wave."""
    grid = g64()
    extra = grid[::4].copy()
    for i in range(len(extra)):
        extra[i]["auto_hot_dice"] = i & 1
        extra[i]["run_up_score"] = (i >> 1) & 1
        if i & 4:
            extra[i]["smart_one"] = 0
        if i & 8:
            extra[i]["smart_one"] = extra[i]["smart_five"] = 0
        extra[i]["favor_score"] = (i >> 2) & 1
        extra[i]["strategy_id"] = 1000 + i
    return np.concatenate([grid, extra])


def two_seat_list(n: int, seed: int = 7):
    """n two-seat games of the mixed table (coords, table, seat_strategy); each altered strategy is seated when n >= 16."""
    rs = np.random.default_rng(seed)
    table = mixed_table()
    coords = make_coords(103, 42, 2, shuffle_index=rs.integers(0, 10**6, size=n), game_index=rs.integers(0, 32, size=n), n=n)
    ss = rs.integers(0, len(table), size=(n, 2))
    m = min(n, 16)
    ss[:m, 1] = 64 + np.arange(m)
    return coords, table, ss.astype(np.int32)


def small_list():
    """The CPU test's list over ONE table (the mixed table + the two scripted tables of tests/golden/watch_vectors.json), as parts
    ``(coords, seat_strategy, k, target_score, max_rounds)``: two-seat games with mixed flags, the three-seat auto_hot_dice game, the
    three-seat run_up_score game with both smart discards, and one game with ``max_rounds = 0``."""
    scripted = gu.load("watch_vectors.json")["scripted"]
    hot, run_up = scripted
    assert hot["name"] == "auto_hot_dice" and run_up["name"] == "run_up_score"
    mixed = mixed_table()
    table = np.concatenate([mixed, gu.strategies_from_tuples(hot["strategies"], STRATEGY_DTYPE),
                            gu.strategies_from_tuples(run_up["strategies"], STRATEGY_DTYPE)])
    coords2, _, ss2 = two_seat_list(20)
    parts = [(coords2, ss2, 2, 10_000, 200)]
    base = len(mixed)
    for case in (hot, run_up):
        coords = make_coords(case["purpose"], case["root_seed"], case["k"], shuffle_index=case["shuffle"], game_index=case["game"])
        parts.append((coords, base + np.arange(case["k"], dtype=np.int32)[None, :], case["k"], case["target"], case["max_rounds"]))
        base += case["k"]
    parts.append((make_coords(103, 9, 2, shuffle_index=1, game_index=2), np.array([[3, 70]], dtype=np.int32), 2, 10_000, 0))
    return table, parts
