"""GPU parity tests of the round-2 device paths, through the C-ABI, against the CPU oracle (bit-exact):

* state-store (GS) game-kernel instances — seat records in the HBM state store, only the turn owner's in LDS — at
  every k, forced on for k = 2 and off for k = 4 (``state_store`` option), every launch geometry;
* result records + ``fk_tally_reduce_kernel`` (LDS-sliced per-(batch, strategy) reduction) and ``fk_tally_direct_kernel``;
* rows produced by the streaming post-pass (``fk_rows_kernel``) from the state store;
* batched H2H blocks (``fk_h2h_run_blocks``): every block equals the serial block loop of the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle

    return pyoracle


def _strats(tuples):
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    return gu.strategies_from_tuples(tuples, STRATEGY_DTYPE)


def _default_table():
    from farkle_ii_amd.strategies import default_grid_tuples

    return _strats(default_grid_tuples())


def _random_valid_table(n: int, seed: int) -> np.ndarray:
    from farkle_ii_amd.strategies import STRATEGY_DTYPE

    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=STRATEGY_DTYPE)
    t["score_threshold"] = rng.integers(2, 21, n) * 50
    t["dice_threshold"] = rng.integers(0, 5, n)
    for name in ("smart_five", "consider_score", "consider_dice", "auto_hot_dice", "run_up_score", "favor_score"):
        t[name] = rng.integers(0, 2, n)
    t["smart_one"] = t["smart_five"] & rng.integers(0, 2, n).astype(np.uint8)
    t["require_both"] = t["consider_score"] & t["consider_dice"] & rng.integers(0, 2, n).astype(np.uint8)
    t["strategy_id"] = np.arange(n)
    return t


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 8, 12])
def test_state_store_and_lds_record_instances_agree_with_oracle(eng, po, k):
    """Same shuffles through the state-store instance, the LDS-record instance (when k records fit) and the oracle:
    tallies per batch, rows.  (The state-store instance is the 768-thread one: the path of tables wider than LDS, k > 64;
    `state_store = 1` selects it at any k.  Its 256- and 64-thread forms were experiment builds and left the tree in round 6.)"""
    table = _random_valid_table(96, 100 + k)
    n_sh = 40
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, 5, 3, 3 + n_sh, shuffles_per_batch=16, want_rows=True, n_threads=8)
    try:
        for store, block in [(1, 0), (0, 0), (-1, 0)]:
            eng.set_option("state_store", store)
            eng.set_option("block", block)
            got = eng.tournament(table, k, 5, 3, 3 + n_sh, shuffles_per_batch=16, want_rows=True)
            assert np.array_equal(got["tally"], ref["tally"]), (k, store, block)
            assert got["rows"].tobytes() == ref["rows"].tobytes(), (k, store, block)
            one = eng.tournament(table, k, 5, 3, 3 + n_sh)  # one batch: LDS tally (96 strategies fit)
            assert np.array_equal(one["tally"][0], ref["tally"].sum(axis=0)), (k, store, block)
            eng.set_option("use_lds_tally", 0)               # ... and the same through result records
            rec = eng.tournament(table, k, 5, 3, 3 + n_sh)
            eng.set_option("use_lds_tally", -1)
            assert np.array_equal(rec["tally"][0], ref["tally"].sum(axis=0)), (k, store, block)
    finally:
        eng.set_option("state_store", -1)
        eng.set_option("block", 0)
        eng.set_option("use_lds_tally", -1)


def test_state_store_limits_overrides_and_safety_games(eng, po):
    """max_rounds / target variants, per-game overrides (sorted + binary search on the device), never-banking tables that
    run to the round limit, max_rounds = 0 — through the state-store instance at k = 4 and k = 2."""
    from farkle_ii_amd.backend import make_overrides

    table = _strats(gu.load("grid_vectors.json")["g64"])
    never = table.copy()
    never["dice_threshold"], never["require_both"] = 0, 1   # every strategy rolls on: all games hit the safety limit
    try:
        for k, store in [(4, -1), (2, 1)]:
            eng.set_option("state_store", store)
            gps = 64 // k
            ovs = [(9, 2, 1, k, 0), (9, 2, 3, k, 7), (9, 5, gps - 1, k, 1), (9, 0, 0, k, 3), (9, 7, 2, k, 250), (9, 2, 5, k, 5)]
            # targets that are not multiples of 50 exercise the unit-of-50 rounding (ceil for "reached", floor for "to beat");
            # 3 200 001 is above what lean records hold (16-bit total / 50): the launch plan falls back to full records
            for tbl, target, mr in [(table, 10_000, 200), (table, 2_000, 5), (never, 10_000, 12), (table, 50, 200), (table, 10_000, 0),
                                    (table, 10_025, 200), (table, 1_030, 60), (table, 75, 200), (table, 1, 200),
                                    (table, 3_200_001, 40), (table, 3_200_000, 40)]:
                ref = po.tournament(tbl.view(po.STRATEGY_DTYPE), k, 9, 0, 10, shuffles_per_batch=3, target_score=target, max_rounds=mr,
                                    overrides=po.make_overrides(ovs), want_rows=True)
                got = eng.tournament(tbl, k, 9, 0, 10, shuffles_per_batch=3, target_score=target, max_rounds=mr,
                                     overrides=make_overrides(ovs), want_rows=True)
                assert np.array_equal(got["tally"], ref["tally"]), (k, target, mr)
                assert got["rows"].tobytes() == ref["rows"].tobytes(), (k, target, mr)
        eng.set_option("state_store", -1)
        with pytest.raises(Exception, match="lean records"):  # the batched head-to-head instance has lean records only
            eng.h2h_blocks(np.stack([table[:2]]), 11, np.array([0], np.uint64), np.array([0], np.uint32), np.array([4], np.uint64),
                           np.array([8], np.uint64), target_score=3_200_001, max_rounds=10)
    finally:
        eng.set_option("state_store", -1)


def test_tally_reduce_slices_on_the_default_grid(eng, po):
    """5 160 strategies: twelve LDS slices per batch part in fk_tally_reduce_kernel (batches of >= 4 096 games), and the
    direct kernel for per-shuffle batches; k = 4 (state store) and k = 2 (LDS records)."""
    table = _default_table()
    for k, n_sh, spb in [(4, 9, 4), (2, 5, 2), (4, 3, 1), (8, 8, 8)]:
        ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, 0, 11, 11 + n_sh, shuffles_per_batch=spb, n_threads=16)
        got = eng.tournament(table, k, 0, 11, 11 + n_sh, shuffles_per_batch=spb)
        assert np.array_equal(got["tally"], ref["tally"]), (k, n_sh, spb)
    # chunked: whole shuffles per chunk, batches straddling chunk boundaries
    try:
        eng.set_option("chunk_bytes", 3 << 20)
        ref = po.tournament(table.view(po.STRATEGY_DTYPE), 4, 0, 0, 10, shuffles_per_batch=4, n_threads=16)
        got = eng.tournament(table, 4, 0, 0, 10, shuffles_per_batch=4)
        assert np.array_equal(got["tally"], ref["tally"])
    finally:
        eng.set_option("chunk_bytes", 48 << 30)


def test_h2h_blocks_batched_equal_serial_blocks(eng, po):
    """Hundreds of (pair, order) blocks in shared launches: mixed strategies incl. never-banking seats (every attempt a
    safety-limit game), per-block targets / attempt caps, resumed states, a chunk limit, overrides."""
    from farkle_ii_amd.backend import make_overrides

    rng = np.random.default_rng(7)
    pool = _random_valid_table(40, 3)
    pool["dice_threshold"][:3], pool["consider_dice"][:3], pool["require_both"][:3], pool["consider_score"][:3] = 0, 1, 1, 1
    n = 300
    seats = np.stack([pool[rng.integers(0, 40, 2)] for _ in range(n)])
    seats[5] = pool[[0, 1]]                        # two never-banking seats: no attempt ever completes
    pair = rng.integers(0, 50, n).astype(np.uint64)
    order = rng.integers(0, 2, n).astype(np.uint32)
    target = rng.integers(1, 160, n).astype(np.uint64)
    max_attempts = (target * rng.choice([1, 2, 3], n)).astype(np.uint64)
    ovs = [(11, int(pair[7]), 3, int(order[7]), 2), (11, int(pair[20]), 0, int(order[20]), 0), (11, int(pair[20]), 5, int(order[20]), 1)]
    for chunk in (None, 37):
        got = eng.h2h_blocks(seats, 11, pair, order, target, max_attempts, chunk_games=chunk, max_rounds=60,
                             overrides=make_overrides(ovs))
        for b in range(n):
            want = po.h2h_block(seats[b].view(po.STRATEGY_DTYPE), 11, int(pair[b]), int(order[b]), int(target[b]), int(max_attempts[b]),
                                int(max_attempts[b]) if chunk is None else chunk, max_rounds=60, overrides=po.make_overrides(ovs))
            assert np.array_equal(got[b], want), (chunk, b, got[b], want)
    assert got[5][1] == 0 and got[5][2] > 0
    # a target that is not a multiple of 50 (the kernels count in units of 50 points)
    got = eng.h2h_blocks(seats[:60], 11, pair[:60], order[:60], target[:60], max_attempts[:60], target_score=2_025, max_rounds=60)
    for b in range(60):
        want = po.h2h_block(seats[b].view(po.STRATEGY_DTYPE), 11, int(pair[b]), int(order[b]), int(target[b]), int(max_attempts[b]),
                            int(max_attempts[b]), target_score=2_025, max_rounds=60)
        assert np.array_equal(got[b], want), (b, got[b], want)
    # resumed blocks: the first chunk's states go back in
    first = eng.h2h_blocks(seats, 11, pair, order, target, max_attempts, chunk_games=25, max_rounds=60)
    second = eng.h2h_blocks(seats, 11, pair, order, target, max_attempts, chunk_games=10**9, max_rounds=60, states=first)
    full = eng.h2h_blocks(seats, 11, pair, order, target, max_attempts, max_rounds=60)
    assert np.array_equal(second, full)
    # more blocks than one launch takes (8 192): 9 000 tiny blocks
    m = 9000
    seats_m = np.stack([pool[[3 + (i % 30), 4 + ((7 * i) % 30)]] for i in range(m)])
    got = eng.h2h_blocks(seats_m, 5, np.arange(m), np.arange(m) % 2, 3, 6, max_rounds=200)
    for b in list(range(0, m, 601)) + [8191, 8192, m - 1]:
        want = po.h2h_block(seats_m[b].view(po.STRATEGY_DTYPE), 5, b, b % 2, 3, 6, 6)
        assert np.array_equal(got[b], want), b
    assert (got[:, 1] == 3).all() or (got[:, 0] == 6).any()


def test_h2h_generations_cut_into_many_pipelined_passes(eng, po):
    """A small workspace budget cuts each generation of a batched H2H call into many launches; blocks straddle passes, the
    next pass is prepared on the side stream while the current one plays (and, with `pipeline` off or overrides present, in
    front of its own game kernel): every block still equals the oracle's serial loop."""
    from farkle_ii_amd.backend import make_overrides

    rng = np.random.default_rng(19)
    pool = _random_valid_table(40, 3)
    pool["dice_threshold"][:3], pool["consider_dice"][:3], pool["require_both"][:3], pool["consider_score"][:3] = 0, 1, 1, 1
    n = 240
    seats = np.stack([pool[rng.integers(0, 40, 2)] for _ in range(n)])
    seats[11] = pool[[0, 2]]
    pair = rng.integers(0, 90, n).astype(np.uint64)
    order = rng.integers(0, 2, n).astype(np.uint32)
    target = rng.integers(40, 900, n).astype(np.uint64)
    max_attempts = (target * 2).astype(np.uint64)
    want = np.stack([po.h2h_block(seats[b].view(po.STRATEGY_DTYPE), 23, int(pair[b]), int(order[b]), int(target[b]), int(max_attempts[b]),
                                  int(max_attempts[b]), max_rounds=80) for b in range(n)])
    ovs = [(23, int(pair[3]), 1, int(order[3]), 0), (23, int(pair[200]), 17, int(order[200]), 2)]
    want_ov = np.stack([po.h2h_block(seats[b].view(po.STRATEGY_DTYPE), 23, int(pair[b]), int(order[b]), int(target[b]), int(max_attempts[b]),
                                     int(max_attempts[b]), max_rounds=80, overrides=po.make_overrides(ovs)) for b in range(n)])
    try:
        for chunk in (1 << 20, 48 << 30):           # ~ 7 000 games per launch: a dozen passes in the first generation / one pass
            eng.set_option("chunk_bytes", chunk)
            for pipeline in (1, 0):
                eng.set_option("pipeline", pipeline)
                got = eng.h2h_blocks(seats, 23, pair, order, target, max_attempts, max_rounds=80)
                assert np.array_equal(got, want), (chunk, pipeline, np.argwhere(got != want)[:4])
                if chunk == 1 << 20:
                    assert eng.timing()["play_launches"] >= 1
            eng.set_option("pipeline", 1)
            got = eng.h2h_blocks(seats, 23, pair, order, target, max_attempts, max_rounds=80, overrides=make_overrides(ovs))
            assert np.array_equal(got, want_ov), chunk
    finally:
        eng.set_option("pipeline", 1)
        eng.set_option("chunk_bytes", 48 << 30)


def test_h2h_production_shape_throughput_sanity(eng):
    """10 000 blocks of 2 191 completed games (the production H2H schedule's block size) in a few launches: every block
    reaches its target, conservation holds, wins are order-symmetric in distribution (not checked bit-wise here)."""
    table = _default_table()
    rng = np.random.default_rng(1)
    n = 10_000
    idx = rng.integers(0, len(table), (n, 2))
    st = eng.h2h_blocks(table[idx], 42, np.arange(n) // 2, np.arange(n) % 2, 2191, 4382)
    assert (st[:, 0] == st[:, 1] + st[:, 2]).all() and (st[:, 1] == st[:, 3] + st[:, 4]).all()
    done = st[:, 1] == 2191
    assert done.mean() > 0.9 and ((st[:, 0] == 4382) | done).all()


def _seat_stats_from_rows(rows: np.ndarray, k: int, S: int, gps: int, spb: int) -> np.ndarray:
    from oracle_engine_stub import seat_stats_from_rows

    return seat_stats_from_rows(rows, k, S, gps, spb)


@pytest.mark.parametrize("k,table_kind", [(2, "g64"), (4, "g64"), (4, "default"), (3, "random")])
def test_all_seat_integer_statistics_match_the_rows(eng, po, k, table_kind):
    """fk_tournament_run_stats: per-(batch, strategy) integer sufficient statistics of all seats, gathered on the device
    from the state store, against the same sums taken over the oracle's rows (incl. safety-limit games and chunking)."""
    table = {"g64": lambda: _strats(gu.load("grid_vectors.json")["g64"]), "default": _default_table,
             "random": lambda: _random_valid_table(96, 5)}[table_kind]()
    S = len(table)
    gps = S // k
    n_sh, spb = (6, 4) if table_kind == "default" else (60, 16)
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, 3, 5, 5 + n_sh, shuffles_per_batch=spb, want_rows=True, max_rounds=40, n_threads=16)
    # the oracle numbers batches from the first shuffle of the call; shuffle 5 is local shuffle 0
    want = _seat_stats_from_rows(ref["rows"], k, S, gps, spb)
    from oracle_engine_stub import seat_ratio_sums_from_rows

    want_ratios = seat_ratio_sums_from_rows(ref["rows"], k, S, gps, spb)
    assert want_ratios[:, :, 0].sum() > 0
    for chunk in (48 << 30, 2 << 20):
        try:
            eng.set_option("chunk_bytes", chunk)
            got = eng.tournament(table, k, 3, 5, 5 + n_sh, shuffles_per_batch=spb, max_rounds=40, want_seat_stats=True, want_rows=True)
        finally:
            eng.set_option("chunk_bytes", 48 << 30)
        assert np.array_equal(got["tally"], ref["tally"])
        assert got["rows"].tobytes() == ref["rows"].tobytes()
        assert got["seat_stats"].shape == want.shape
        assert np.array_equal(got["seat_stats"], want), (k, table_kind, chunk, np.argwhere(got["seat_stats"] != want)[:5])
        # the four float64 sums (fk_tournament_run_all_player): the reference's np.add.at order — BIT equality, also when a batch
        # straddles chunks (the running sums continue on the device)
        assert got["seat_ratio_sums"].tobytes() == want_ratios.tobytes(), (k, table_kind, chunk, np.argwhere(got["seat_ratio_sums"] != want_ratios)[:5])
    assert want[:, :, 2].sum() > 0 or (k, table_kind) != (2, "g64")  # the 64-grid's never-banking pairings hit the 40-round limit
    only = eng.tournament(table, k, 3, 5, 5 + n_sh, shuffles_per_batch=spb, max_rounds=40, want_seat_stats=True)
    assert np.array_equal(only["seat_stats"], want)


def test_rccl_tally_reduce_through_the_c_abi_single_rank(eng):
    """fk_comm_unique_id / fk_comm_init / fk_reduce_tally / fk_comm_destroy on a one-rank communicator (the box has one
    GPU): librccl is loaded at run time, ncclReduce(sum, int64) runs on the engine's stream, and the tally comes back
    unchanged; the engine keeps working afterwards.  Multi-rank use is the same calls with world > 1."""
    from farkle_ii_amd.backend import FarkleHipError

    rng = np.random.default_rng(0)
    tally = rng.integers(0, 2**40, (3, 64, 26), dtype=np.int64)
    with pytest.raises(FarkleHipError, match="no communicator"):
        eng.reduce_tally(tally)
    eng.comm_init(eng.comm_unique_id(), 0, 1)
    try:
        assert np.array_equal(eng.reduce_tally(tally, 0), tally)
        big = rng.integers(0, 2**50, (5160, 26), dtype=np.int64)
        assert np.array_equal(eng.reduce_tally(big, 0), big)
    finally:
        eng.comm_destroy()
    table = _strats(gu.load("grid_vectors.json")["g64"])
    assert eng.tournament(table, 2, 42, 0, 4)["tally"].sum() > 0


def test_rows_leave_in_overlapped_chunks_into_pageable_and_pinned_buffers(eng, po):
    """Rows mode plays in several chunks per call; the rows of chunk i cross PCIe on a copy stream (two device row buffers)
    while chunk i + 1 plays, into a caller buffer that may be page-locked (Engine.pinned_empty -> fk_host_alloc) or not.  Rows,
    tallies and all-seat statistics equal the oracle's whatever the chunking; k = 2 / 3 / 8 cover the staged row kernel's tile
    shapes."""
    from farkle_ii_amd.backend import row_dtype

    try:
        for k, S, n_sh, chunk in [(2, 96, 70, 300), (3, 96, 33, 64), (8, 96, 21, 50), (2, 96, 9, 10**9)]:
            table = _random_valid_table(S, 40 + k)
            ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, 3, 5, 5 + n_sh, shuffles_per_batch=7, want_rows=True, n_threads=8)
            eng.set_option("rows_chunk_games", chunk)
            got = eng.tournament(table, k, 3, 5, 5 + n_sh, shuffles_per_batch=7, want_rows=True, want_seat_stats=True)
            assert got["rows"].tobytes() == ref["rows"].tobytes() and np.array_equal(got["tally"], ref["tally"]), (k, chunk)
            pinned = eng.pinned_empty(n_sh * (S // k) + 5, row_dtype(k))
            pinned[:] = np.zeros(1, dtype=row_dtype(k))[0]
            again = eng.tournament(table, k, 3, 5, 5 + n_sh, shuffles_per_batch=7, want_rows=True, want_seat_stats=True, rows_out=pinned)
            assert again["rows"].tobytes() == ref["rows"].tobytes() and np.array_equal(again["seat_stats"], got["seat_stats"]), (k, chunk)
            assert np.shares_memory(again["rows"], pinned)
            with pytest.raises(ValueError, match="rows_out"):
                eng.tournament(table, k, 3, 5, 5 + n_sh, want_rows=True, rows_out=pinned[:3])
    finally:
        eng.set_option("rows_chunk_games", 4_000_000)


def test_resident_tally_accumulates_on_the_device_and_reduces_through_rccl(eng):
    """Option resident_tally: every tournament call adds its tally to an accumulator in HBM; fk_tally_resident_reduce sums it
    over the communicator on the device (here: none, then a one-rank RCCL communicator), returns it on the root and clears it."""
    table = _strats(gu.load("grid_vectors.json")["g64"])
    try:
        eng.set_option("resident_tally", 1)
        a = eng.tournament(table, 2, 42, 0, 50)["tally"]
        b = eng.tournament(table, 2, 42, 50, 120)["tally"]
        assert np.array_equal(eng.reduce_resident_tally(a.shape), a + b)      # no communicator: the plain copy
        c = eng.tournament(table, 2, 42, 120, 130)["tally"]
        assert np.array_equal(eng.reduce_resident_tally(c.shape), c)          # ... which cleared the accumulator
        assert eng.comm_ranks() == 1
        eng.comm_init(eng.comm_unique_id(), 0, 1)
        try:
            assert eng.comm_ranks() == 1                                       # ncclCommCount
            d = eng.tournament(table, 4, 7, 0, 30, shuffles_per_batch=10)["tally"]  # another shape: a new accumulator
            e = eng.tournament(table, 4, 7, 30, 60, shuffles_per_batch=10)["tally"]
            assert np.array_equal(eng.reduce_resident_tally(d.shape, 0), d + e)
            with pytest.raises(Exception, match="resident tally holds"):
                eng.reduce_resident_tally((5, 5))
        finally:
            eng.comm_destroy()
        # a call that the hot / cold kernel hands back (a counter reaches its guard bit) and the C-ABI replays on the LDS-record
        # kernel joins the accumulator ONCE; a call that fails (1000-roll fuse cannot be provoked here: a bad argument) not at all
        never = table[:8].copy()
        never["dice_threshold"], never["require_both"], never["auto_hot_dice"], never["strategy_id"] = 0, 1, 1, np.arange(8)
        f = eng.tournament(never, 4, 3, 0, 2, max_rounds=6000)["tally"]        # replayed (tests/test_hot_cold_gpu.py)
        g = eng.tournament(never, 4, 3, 2, 5, max_rounds=40)["tally"]
        with pytest.raises(Exception):
            eng.tournament(never, 4, 3, 5, 4)                                 # empty / inverted range
        assert np.array_equal(eng.reduce_resident_tally(f.shape), f + g)
    finally:
        eng.set_option("resident_tally", 0)


@pytest.mark.parametrize("S,k", [(8, 2), (64, 2), (96, 3), (1290, 2), (5160, 4), (7140, 5), (16386, 2), (32770, 2), (65534, 2)])
def test_permutation_kernels_agree_with_numpy_semantics(eng, po, S, k):
    """Generator.permutation through the three device paths — one-kernel Fisher-Yates, draws + serial swap chains, draws +
    the chain-free kernel (bucket sort + pointer jumping), the draws by a thread or by a wave per shuffle — against the oracle's
    restatement of NumPy's loop, permutations and tallies; shuffle counts that leave partial blocks and partial 8-draw groups.
    16 386 / 32 770 / 65 534 strategies (k = 2): the masked draws of a shuffle change bit length between the bounds 16 383 / 16 384 and
    32 767 / 32 768, and 65 534 is the largest table the ABI takes; at these sizes the chain-free kernel's LDS does not fit, so split
    modes 1 and 2 both run the swap chains.
    Odd tables, every tail of the last draw group, the LDS seams and synthetic draw lists: test_perm_stage_gpu.py / perm_stage_cases.py."""
    table = _random_valid_table(S, S) if (S <= 96 or S > 5160) else _default_table()[:S]  # 7 140: the reference's largest documented grid
    n_sh = {8: 300, 64: 521, 96: 77, 1290: 70, 5160: 37, 7140: 260, 16386: 5, 32770: 4, 65534: 3}[S]
    ref = po.tournament(table.view(po.STRATEGY_DTYPE), k, 21, 1000, 1000 + n_sh, want_perms=True, max_rounds=3, n_threads=16)
    try:
        for mode in (0, 1, 2, -1):
            eng.set_option("perm_split", mode)
            # the draws of the two split paths: by one thread per shuffle (0) or by a whole wave (1: jump-ahead by 64 + the rejection
            # scan iterated to its fixed point, csrc/fk_perm_wave.h) — the same 16-bit draws in the same groups
            for draw_by_wave in ((0, 1) if mode >= 0 else (-1,)):
                eng.set_option("perm_draw_wave", draw_by_wave)
                try:
                    got = eng.tournament(table, k, 21, 1000, 1000 + n_sh, want_perms=True, max_rounds=3)
                except Exception as exc:
                    raise AssertionError(f"perm_split={mode} S={S}: {exc}") from exc
                assert np.array_equal(got["perms"], ref["perms"]), (S, mode, draw_by_wave, np.argwhere(got["perms"] != ref["perms"])[:4])
                assert np.array_equal(got["tally"], ref["tally"]), (S, mode, draw_by_wave)
    finally:
        eng.set_option("perm_split", -1)
        eng.set_option("perm_draw_wave", -1)


def test_pipelined_preparation_never_changes_results(eng, po):
    """The next chunk's (or the hinted next call's) permutations run in front of the current game kernel and its seat seeding on a
    side stream behind it.  Same results with the pipeline on (the default) and off, for multi-chunk calls, right hints, wrong hints, hints followed by other entry
    points, a table change after a hint, rows / statistics calls."""
    from farkle_ii_amd.backend import make_coords

    table = _strats(gu.load("grid_vectors.json")["g64"])
    other = _random_valid_table(96, 11)
    ref = {rng: po.tournament(table.view(po.STRATEGY_DTYPE), 2, 42, rng[0], rng[1], want_rows=True, n_threads=16)
           for rng in [(0, 600), (600, 1200), (1200, 1500), (77, 300)]}
    ref_other = po.tournament(other.view(po.STRATEGY_DTYPE), 3, 42, 600, 900, n_threads=16)

    def check(rng, hinted=False, **kw):
        got = eng.tournament(table, 2, 42, rng[0], rng[1], **kw)
        assert np.array_equal(got["tally"], ref[rng]["tally"]), (rng, kw)
        if kw.get("want_rows"):
            assert got["rows"].tobytes() == ref[rng]["rows"].tobytes(), (rng, kw)
        if hinted:  # the call a right hint was made for: its first chunk was prepared behind the previous call's game kernel, the others behind its own
            t = eng.timing()
            assert t["prefetched_chunks"] == (t["play_launches"] if pipeline else 0), (rng, kw, pipeline, chunk, t)

    try:
        for pipeline in (1, 0):
            eng.set_option("pipeline", pipeline)
            for chunk in (48 << 30, 400 << 10):   # one chunk / about ten chunks per call
                eng.set_option("chunk_bytes", chunk)
                eng.hint_next(600, 1200)            # right hint
                check((0, 600))
                eng.hint_next(1200, 1500, need_state=True)
                check((600, 1200), hinted=True)
                # (a rows call's chunks are shorter than the plain call's that prepared for it: only a one-chunk call finds its chunk)
                check((1200, 1500), hinted=chunk == 48 << 30, want_rows=True)
                eng.hint_next(0, 600)               # wrong hint: another range is played
                check((77, 300), want_rows=True)
                check((0, 600))                     # ... and the hinted one after all, a call later
                eng.hint_next(600, 1200)            # hint, then other entry points use the context
                check((0, 600))
                coords = make_coords(10, 5, 2, 0, 0, 0, np.arange(50, dtype=np.uint64))
                rows = eng.play_games(coords, table, np.tile(np.arange(2, dtype=np.int32), (50, 1)), 2)
                want = po.play_games(coords.view(po.COORD_DTYPE), table.view(po.STRATEGY_DTYPE), np.tile(np.arange(2, dtype=np.int32), (50, 1)), 2)
                assert rows.tobytes() == want.tobytes()
                check((600, 1200))
                eng.hint_next(600, 900)             # hint, then the table changes
                check((0, 600))
                got = eng.tournament(other, 3, 42, 600, 900)
                assert np.array_equal(got["tally"], ref_other["tally"])
                check((600, 1200), want_seat_stats=True)
    finally:
        eng.set_option("pipeline", 1)
        eng.set_option("chunk_bytes", 48 << 30)


def test_comm_init_with_a_peer_that_never_joins_returns_fk_err_comm_within_the_deadline():
    """A world of two whose second rank never calls in: `fk_comm_init` (non-blocking ncclCommInitRankConfig polled under
    `comm_timeout_ms`) must come back with FK_ERR_COMM, abort the half-made communicator and leave the engine usable — in a child
    process, which then exits.  (Round 3's blocking ncclCommInitRank would sit there until the job's time limit.)"""
    import subprocess
    import sys
    import time
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    child = f"""
import sys, time
sys.path.insert(0, {str(root)!r})
import numpy as np
from farkle_ii_amd.backend import Engine, FarkleHipError, FK_ERR_COMM
from bench import grid64
eng = Engine(0)
eng.set_option("comm_timeout_ms", 4000)
t0 = time.time()
try:
    eng.comm_init(eng.comm_unique_id(), 0, 2)
except FarkleHipError as exc:
    assert exc.code == FK_ERR_COMM, exc
    assert "comm_timeout_ms" in str(exc) or "ncclCommInitRank" in str(exc), exc
    print("refused after %.1f s: %s" % (time.time() - t0, exc))
else:
    raise SystemExit("fk_comm_init returned success for a world of two with one rank")
assert time.time() - t0 < 60
assert eng.comm_ranks() == 1
assert eng.tournament(grid64(), 2, 42, 0, 4)["tally"].sum() > 0   # the context still plays
eng.close()
print("child ok")
"""
    import os
    import re

    # an explicit option wins over the environment default (round-4 advisor: FK_COMM_TIMEOUT_MS used to override it silently)
    t0 = time.time()
    res = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=150, cwd=str(root),
                         env=dict(os.environ, FK_COMM_TIMEOUT_MS="1"))
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    assert time.time() - t0 < 120  # the timed-out process ends by itself, helper thread inside librccl and all
    assert float(re.search(r"refused after ([0-9.]+) s", res.stdout).group(1)) >= 3.5, res.stdout
    # the environment default alone (option never set), and a malformed value is ignored instead of selecting the blocking call
    env_child = child.replace('eng.set_option("comm_timeout_ms", 4000)\n', "")
    assert env_child != child
    res = subprocess.run([sys.executable, "-c", env_child], capture_output=True, text=True, timeout=150, cwd=str(root),
                         env=dict(os.environ, FK_COMM_TIMEOUT_MS="2500"))
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    assert 2.0 <= float(re.search(r"refused after ([0-9.]+) s", res.stdout).group(1)) < 30, res.stdout
    # Malformed FK_COMM_TIMEOUT_MS values fall back to the 120-s DEFAULT — not to 0, which would select the blocking path (round-5
    # advisor: the earlier probe set the option first, so the parser never ran).  One child per value, no set_option call; the effective
    # deadline is read back through fk_get_option ("comm_timeout_ms").
    probe = f"""
import sys
sys.path.insert(0, {str(root)!r})
from farkle_ii_amd.backend import Engine
eng = Engine(0)
print("effective", eng.get_option("comm_timeout_ms"))
eng.set_option("comm_timeout_ms", 1500)
print("after set_option", eng.get_option("comm_timeout_ms"))
eng.close()
"""
    for raw, want in (("-5", 120000), ("12x", 120000), ("", 120000), ("99999999999", 120000), ("0", 0), ("2500", 2500)):
        res = subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, timeout=150, cwd=str(root),
                             env=dict(os.environ, FK_COMM_TIMEOUT_MS=raw))
        assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
        assert int(re.search(r"effective (-?[0-9]+)", res.stdout).group(1)) == want, (raw, res.stdout)
        assert int(re.search(r"after set_option ([0-9]+)", res.stdout).group(1)) == 1500, (raw, res.stdout)  # an explicit option wins
