"""TEST INFRASTRUCTURE ONLY — strategy tables whose games are decided before they are played, and the cases the decided-table tests
(`test_decided_tables_cpu.py`, `test_decided_tables_gpu.py`) share.

A row of ``decided_table(S, bankers)`` outside ``bankers`` never banks: ``dice_threshold = 0`` with ``consider_dice = consider_score =
require_both = 1`` rolls on while dice are left (`fko_decide`: ``want_s || want_d``, and a decision is only taken with a die in hand),
the recipe of ``round_robin_engine_stub.hard_table``.  Here ``run_up_score = 1`` is part of it: in the final round every seat rolls
until it has passed the leader, and a seat WITHOUT ``run_up_score`` stops there and banks, so such a "never-banker" wins the odd game
with one turn worth more than the target (3 of 29 mirrored couples of one pair, 1 of 9 867 games of ``edge1794``, measured with the
flag left as the grids have it).  With the flag it rolls on until it farkles: its score is 0 in every row, it never wins, and a game
of never-bankers alone always runs to the round limit.

A row IN ``bankers`` keeps the grid's strategy, except that the grids hold never-bankers of their own (rows 0, 1, 16, 17, 32, 33, 48, 49
of the 64-strategy grid, 184 of the first 1 794 default-grid rows, row 0 among them): a banker row of that form has ``require_both``
cleared, which makes it bank at its score threshold.

``TARGET_SCORE`` / ``MAX_ROUNDS`` / ``ROOT_SEED`` are the values under which every condition of `test_decided_tables_cpu.py` holds;
they are the issue's starting values, none had to move."""
from __future__ import annotations

import numpy as np

TARGET_SCORE = 2000
MAX_ROUNDS = 12
ROOT_SEED = 3
PLAY = dict(target_score=TARGET_SCORE, max_rounds=MAX_ROUNDS)

# tally columns (include/farkle_hip.h) and lag-sum columns (rng_lags._pair_sums) the conditions read
WINS, GAMES, COMPLETED, SAFETY = 0, 1, 2, 3
LAG_PAIRS, LAG_WX, LAG_WY, LAG_WXY = 0, 1, 2, 5

EDGE_S = 1794                          # slices of 896, 896 and 2 strategies in fk_tally_reduce_kernel
EDGE_WINNERS = (0, 895, 896, 1791, 1793)
EDGE_RANGE = dict(shuffle_begin=5, shuffle_end=16, shuffles_per_batch=5)  # 897 games a shuffle: 4 485 a batch; two full batches and one shuffle


def base_table(S: int) -> np.ndarray:
    """The first ``S`` rows of the seat-analysis fixture grid (up to twelve), of the 64-strategy grid, or of the default grid."""
    if S <= 12:
        from test_seat_analysis_cpu import CASES, case_table

        return case_table(CASES[0])[0][:S].copy()
    from tools.time_config import table_for

    return table_for(64)[:S].copy() if S <= 64 else table_for(S).copy()


def never_banks(table: np.ndarray) -> np.ndarray:
    """Rows that roll on at every decision outside the final round: the dice test always asks for more and nothing overrules it."""
    always_dice = (table["consider_dice"] == 1) & (table["dice_threshold"] < 1)
    return always_dice & ((table["consider_score"] == 0) | (table["require_both"] == 1))


def decided_table(S: int, bankers) -> np.ndarray:
    table = base_table(S)
    keep = np.zeros(S, dtype=bool)
    keep[np.asarray(sorted(bankers), dtype=np.int64)] = True
    table["dice_threshold"][~keep] = 0
    for name in ("consider_dice", "consider_score", "require_both", "run_up_score"):
        table[name][~keep] = 1
    table["require_both"][keep & never_banks(table) & (table["consider_score"] == 1)] = 0
    assert np.array_equal(never_banks(table), ~keep)
    return table


def half12_ids() -> np.ndarray:
    """Unique IDs whose order is not the table's (``_ids`` of `test_seat_analysis_gpu.py`)."""
    return ((np.arange(12, dtype=np.int64) * 37 + 11) % 257).astype(np.int32)


def half12_bankers() -> list[int]:
    rank = np.argsort(np.argsort(half12_ids()))
    return [int(i) for i in np.nonzero(rank % 2 == 0)[0]]


TABLES = {
    "none64": lambda: decided_table(64, ()),
    "one64": lambda: decided_table(64, (17,)),
    "half12": lambda: decided_table(12, half12_bankers()),
    "half64": lambda: decided_table(64, range(0, 64, 2)),
}
SEATS = {"none64": (2, 4), "one64": (2,), "half12": (2,), "half64": (2, 4)}


def table(name: str) -> np.ndarray:
    return TABLES[name]()


def edge_table(winner: int) -> np.ndarray:
    return decided_table(EDGE_S, (winner,))


# the runs both modules make: positional (k, root_seed, shuffle_begin, shuffle_end) and keywords
TALLY_BATCHED = dict(shuffle_begin=0, shuffle_end=40, shuffles_per_batch=16)
HALF12_PAIRS = dict(shuffle_begin=0, shuffle_end=700, shuffles_per_batch=300)
HALF64_PAIRS = dict(shuffle_begin=0, shuffle_end=96, shuffles_per_batch=32)
LAGS = (1, 3, 7)
LAG_SHUFFLES = 200
ONE64_ALWAYS_ROUNDS = 20        # the one addition to MAX_ROUNDS: with twenty rounds the lone banker of one64 wins all 200 shuffles
RARE_TARGET = 1500              # bankers end their won games at 2 000 or more, and lose some at 1 500 or more
DENSE_THRESHOLDS = (-50, 2 ** 31 - 1)  # flags every completed game (`test_hip_dense_and_empty_lists`)


def run(engine, method: str, tbl: np.ndarray, k: int, shuffle_begin: int, shuffle_end: int, *args, **kw):
    return getattr(engine, method)(tbl, k, ROOT_SEED, shuffle_begin, shuffle_end, *args, **{**PLAY, **kw})


def pair_kinds(sums: np.ndarray) -> dict:
    """How many mirrored-pair rows are of each decided kind (columns: ``seat_analysis.PAIR_COLUMNS``)."""
    paired, diff, completed, safety = (sums[:, c] for c in range(4))
    return {"all_plus": int(((diff == paired) & (paired > 0)).sum()), "all_minus": int(((diff == -paired) & (paired > 0)).sum()),
            "none_completed": int(((completed == 0) & (safety > 0)).sum()),
            "between": int(((np.abs(diff) > 0) & (np.abs(diff) < paired)).sum())}
