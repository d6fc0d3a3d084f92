"""TEST INFRASTRUCTURE ONLY — tournaments of 13 to 128 seats: the player counts at which the library changes shape beyond the
reference's production list (which ends at twelve), one case per count, each case's expected result (the CPU oracle, computed
once per process and never changed by a test), the preconditions on that result which prove the case reaches both outcomes of a
game, and the launch-plan / row-tile arithmetic of csrc restated from the constants the sources hold (test helper, not a conftest).

    13   past the hot / cold kernel: fk_play_kernel at a run-time seat count, 256-thread lean; rows tile of 128 lanes
    16   lean records fill LDS to the byte (256 x 16 x 40 = 163 840); last count of seat counts and matchup records
    17   64-thread blocks, three per CU; column images by one thread per game
    19   rows tile of 64 lanes
    32   LDS filled to the byte again (128 x 32 x 40)
    33, 37   full 17-dword records win the plan's tie-break; 37 is the last count whose full records fit
    37   a row is longer than 1 024 bytes: the rows kernel without an LDS tile
    38   full records no longer fit: `lean = 0` plays on the state-store instance, a target beyond lean records is refused
    64   LDS filled to the byte, one wave per CU; last count of column images
    65   the state-store instance by the plan's own choice
    128  the last seat a row can name (int8 winner_seat, seven bits of the result word)
"""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np

import kernel_instances as ki
from oracle_engine_stub import po, seat_ratio_sums_from_rows, seat_stats_from_rows

KS = (13, 16, 17, 19, 32, 33, 37, 38, 64, 65, 128)
MAX_PLAYERS = 128  # FK_MAX_PLAYERS of include/farkle_hip.h (test_wide_tables_cpu.py reads the header)
ROOT, BEGIN, SPB = 5, 3, 16
RARE_THRESHOLDS = (500, 1000)
POST_PASS_KS = (13, 17, 37, 64, 65)
COLUMN_KS = (13, 16, 17, 37, 64)
BEYOND_LEAN = 3_200_001  # one point above 50 * LEAN_MAX_TARGET50: lean records cannot carry the banked total


def table_size(k: int) -> int:
    return k * (8 if k <= 17 else 3 if k <= 33 else 2 if k <= 65 else 1)


def n_shuffles(k: int) -> int:
    return 40 if k <= 54 else 200 if k <= 65 else 600


def max_rounds(k: int) -> int:
    return 12 if k == 128 else 14


@lru_cache(maxsize=None)
def table(k: int) -> np.ndarray:
    t = ki._random_legal(table_size(k), 7 + k)
    ki.check_legal(t)
    t.setflags(write=False)
    return t


def ids(S: int) -> np.ndarray:
    """Unique strategy IDs (S <= 257), negative ones among them, whose order is not the table's: they wrap every three rows."""
    assert S <= 257
    return ((np.arange(S, dtype=np.int64) * 97 + 11) % 257 - 100).astype(np.int32)


def call(k: int, **extra) -> dict:
    """The arguments of case k after the table and k (``Engine.tournament`` and every stub take them by these names)."""
    return dict(dict(root_seed=ROOT, shuffle_begin=BEGIN, shuffle_end=BEGIN + n_shuffles(k), shuffles_per_batch=SPB, max_rounds=max_rounds(k)),
                **extra)


@lru_cache(maxsize=None)
def want(k: int) -> dict:
    """The oracle's result of case k: perms, rows, per-batch tally, and the all-seat statistics summed from its rows."""
    t = table(k)
    res = po.tournament(t.view(po.STRATEGY_DTYPE), k, ROOT, BEGIN, BEGIN + n_shuffles(k), shuffles_per_batch=SPB, max_rounds=max_rounds(k),
                        want_rows=True, want_perms=True, n_threads=4)
    S = len(t)
    out = {"tally": res["tally"], "rows": res["rows"], "perms": res["perms"],
           "seat_stats": seat_stats_from_rows(res["rows"], k, S, S // k, SPB),
           "seat_ratio_sums": seat_ratio_sums_from_rows(res["rows"], k, S, S // k, SPB)}
    for v in out.values():
        v.setflags(write=False)
    return out


def figures(k: int) -> dict:
    rows = want(k)["rows"]
    done = rows["status"] == 0
    winners = rows["winner_seat"][done].astype(np.int64)
    return {"games": len(rows), "completed": int(done.sum()), "safety": int((~done).sum()), "seat0_wins": int((winners == 0).sum()),
            "last_seat_wins": int((winners == k - 1).sum()), "wins_at_64_up": int((winners >= 64).sum()),
            "batches": len(want(k)["tally"]), "last_batch": n_shuffles(k) % SPB}


def check_preconditions(k: int) -> dict:
    """The oracle's result of case k reaches both outcomes of a game and both ends of the table; -> its figures."""
    fig = figures(k)
    assert fig["games"] == n_shuffles(k) * (table_size(k) // k) and fig["completed"] + fig["safety"] == fig["games"]
    assert 20 * fig["completed"] >= fig["games"] and 20 * fig["safety"] >= fig["games"], fig  # each at least 5 % of the games
    assert fig["seat0_wins"] >= 1 and fig["last_seat_wins"] >= 1, fig
    if k == 128:
        assert fig["wins_at_64_up"] >= 1 and fig["last_seat_wins"] >= 1, fig  # the seventh seat bit in use, and seat 127 itself
    assert fig["last_batch"] != 0 and fig["batches"] == n_shuffles(k) // SPB + 1  # a ragged last batch
    assert np.all(want(k)["rows"]["winner_seat"][want(k)["rows"]["status"] == 1] == -1)
    return fig


# ------------------------------------------------------------------------------------- the sources' constants and arithmetic
CSRC = Path(__file__).resolve().parent.parent / "farkle_ii_amd" / "csrc"


@lru_cache(maxsize=None)
def constants() -> dict:
    """LDS_LIMIT, the record sizes, the rows tile and the limits, read out of the sources (so that a change there shows here)."""
    hip = (CSRC / "farkle_hip.hip").read_text()
    kern = (CSRC / "fk_kernels.h").read_text()
    hc = (CSRC / "fk_play_hc.h").read_text()

    def one(pattern: str, text: str) -> str:
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]

    a, b = one(r"constexpr size_t LDS_LIMIT = (\d+) \* (\d+);", hip)
    fields = one(r"enum : uint32_t \{\s*(F_LO0 = 0,[^}]*?), NF\s*\};", kern)
    tile = set(re.findall(r"\(size_t\)block \* row_dw \* 4 > (\d+)\)|if \(tile <= (\d+)\)", hip))
    assert tile == {("65536", ""), ("", "65536")}, tile
    return {"LDS_LIMIT": int(a) * int(b), "LEAN_BYTES": 4 * int(one(r"constexpr uint32_t LEAN_DW = (\d+);", kern)),
            "FULL_BYTES": 4 * len([f for f in fields.replace("\n", " ").split(",") if f.strip()]),
            "LEAN_MAX_TARGET50": int(one(r"constexpr int32_t LEAN_MAX_TARGET50 = (\d+);", kern)),
            "LT_COLS": int(one(r"constexpr uint32_t LT_COLS = (\d+);", kern)), "CE_IDX_SHIFT": int(one(r"constexpr uint32_t CE_IDX_SHIFT = (\d+);", kern)),
            "HC_MAX_K": int(one(r"constexpr uint32_t HC_MAX_K = (\d+);", hc)), "ROWS_TILE": 65536,
            "ROWS_FIRST_BLOCK": int(one(r"uint32_t block = (\d+);\s*while \(block > 64 &&", hip))}


def record_lds_bytes(k: int, block: int, lean: bool, gs: bool, tally: bool, S: int) -> int:
    """``row_lds_bytes`` of csrc/fk_plan.h for an LDS-record row, plus the LDS tally."""
    c = constants()
    return (c["LEAN_BYTES"] if lean else c["FULL_BYTES"]) * (1 if gs else k) * block + (S * c["LT_COLS"] * 8 if tally else 0)


def plan(k: int, S: int, single_batch: bool = False, target_score: int = 10_000, lean: int = -1, state_store: int = -1,
         use_lds_tally: int = -1, max_waves: int = 6) -> dict | None:
    """``plan_play`` of csrc/fk_plan.h (its LDS-record part) for a tournament launch under the options a test sets (block / blocks_per_cu at their
    defaults): the most resident lanes per CU; ties go to an LDS tally, then to full records, then to the larger block.  ``None``:
    no instance."""
    c = constants()
    limit = c["LDS_LIMIT"]
    lean_ok = (target_score + 49) // 50 <= c["LEAN_MAX_TARGET50"]
    want_tally = single_batch and use_lds_tally != 0 and S <= 4096
    best, best_lanes = None, -1
    wanted = 1 if state_store == 1 else 0
    for gs in (0, 1):
        if gs != wanted and best_lanes >= 0:
            continue
        for ln in (0, 1):
            if (gs and not ln) or (ln and not lean_ok) or (not gs and lean >= 0 and ln != lean):
                continue
            if not gs and ln and S > 1 << (32 - c["CE_IDX_SHIFT"]):
                continue
            for block in (1024, 768, 512, 256, 128, 64):
                if (gs and block != 768) or (block == 768 and not ln):
                    continue
                tally = want_tally and record_lds_bytes(k, block, bool(ln), bool(gs), True, S) <= limit // (2 if gs else 1)
                lds = record_lds_bytes(k, block, bool(ln), bool(gs), tally, S)
                if lds > limit:
                    continue
                per_cu = max(min(limit // max(lds, 1), max(1, max_waves * 4 * 64 // block)), 1)
                lanes = per_cu * block * 4 + (2 if tally else 0) + (0 if ln else 1) + ((1 << 24) if gs == wanted else 0)
                if lanes > best_lanes:
                    best_lanes = lanes
                    best = {"block": block, "lean": bool(ln), "gs": bool(gs), "lds": lds, "tally": tally, "per_cu": per_cu}
    return best


def rows_tile_lanes(k: int) -> int:
    """The rows launch of csrc/farkle_hip.hip (``rows_pass``): the lanes of the LDS tile a block's rows leave through; 0 = the
    kernel without a tile (one thread stores its own row)."""
    c = constants()
    block = c["ROWS_FIRST_BLOCK"]
    while block > 64 and block * (4 + 28 * k) > c["ROWS_TILE"]:
        block -= 64
    return block if block * (4 + 28 * k) <= c["ROWS_TILE"] else 0


def instance_args(instance: str) -> list[str]:
    """``fk_play_kernel<256, true, 4, 65280u, false, false, 0>`` -> its template arguments; not a hot / cold instance."""
    assert instance.startswith("fk_play_kernel<") and instance.endswith(">"), instance
    return instance[len("fk_play_kernel<"):-1].split(", ")
