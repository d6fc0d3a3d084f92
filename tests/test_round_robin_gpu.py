"""``fk_h2h_round_robin`` on the MI355X against the oracle, bit for bit: block states and the per-strategy summary of the HIP engine
equal the entry restated on the CPU oracle (tests/round_robin_engine_stub.py: itertools pairs, the oracle's ``h2h_block`` per block, the
summary in NumPy) — under every window size, workspace budget and pipeline setting, over pair ranges, against the explicit-block path
(``fk_h2h_run_blocks``), at the smallest tables, after every refusal, and on a wide table of one-attempt blocks."""
from __future__ import annotations

import numpy as np
import pytest

import round_robin_engine_stub as stub

pytestmark = pytest.mark.gpu

HARD = stub.HARD
N_PAIRS = 66  # 12 strategies


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    return stub.Engine(0)


@pytest.fixture(scope="module")
def table():
    return stub.hard_table()


@pytest.fixture(scope="module")
def hard_ref(oracle, table):
    """The hard case on the oracle, computed once; with the properties that make it hard asserted on the oracle's own result."""
    states, summary = oracle.h2h_round_robin(table, **HARD)
    flat = states.reshape(-1, 5).astype(np.int64)
    target = HARD["target"]
    multi_generation = int(((flat[:, 1] >= target) & (flat[:, 2] > 0)).sum())   # reached the target with safety-limit games in between
    unresolved_partial = int(((flat[:, 1] < target) & (flat[:, 1] > 0)).sum())
    zero_completed = int((flat[:, 1] == 0).sum())
    assert len(flat) == 132 and multi_generation >= 50 and unresolved_partial >= 5 and zero_completed >= 2
    states.setflags(write=False)
    summary.setflags(write=False)
    return states, summary


def _with_options(eng, options: dict, call):
    saved = {name: eng.get_option(name) for name in options if name in ("chunk_bytes", "rr_window_blocks")}
    try:
        for name, value in options.items():
            eng.set_option(name, value)
        return call()
    finally:
        for name in options:
            eng.set_option(name, saved[name] if name in saved else {"pipeline": 1}[name])


@pytest.mark.parametrize("window", [None, 32, 2])
@pytest.mark.parametrize("chunk_bytes", [None, 1 << 20])
@pytest.mark.parametrize("pipeline", [1, 0])
def test_hard_case_under_every_schedule(eng, table, hard_ref, window, chunk_bytes, pipeline):
    """Multi-generation, unresolved and never-completing blocks; windows that split the range; both preparation modes."""
    options = {"pipeline": pipeline}
    if window is not None:
        options["rr_window_blocks"] = window
    if chunk_bytes is not None:
        options["chunk_bytes"] = chunk_bytes
    states, summary = _with_options(eng, options, lambda: eng.h2h_round_robin(table, **HARD))
    assert states.dtype == np.uint32 and states.shape == (N_PAIRS, 2, 5) and summary.dtype == np.int64 and summary.shape == (12, 8)
    assert np.array_equal(states, hard_ref[0]) and np.array_equal(summary, hard_ref[1])
    t = eng.timing()
    assert t["games"] == int(hard_ref[0][:, :, 0].sum()) and t["play_launches"] >= 2  # (at least two generations)
    assert eng.last_play_instance().startswith("fk_play_kernel<")


@pytest.mark.parametrize("pipeline", [1, 0])
def test_passes_that_cut_blocks(eng, oracle, table, pipeline):
    """Longer blocks under the smallest workspace budget: a generation of 132 x 400 games is several launches (a 1-MiB budget holds
    about 12 483 two-seat games), blocks straddle them, and pass i + 1 is prepared around pass i."""
    call = dict(root_seed=11, target=400, max_attempts=800, max_rounds=24)
    want = oracle.h2h_round_robin(table, **call)
    got = _with_options(eng, {"chunk_bytes": 1 << 20, "pipeline": pipeline}, lambda: (eng.h2h_round_robin(table, **call), eng.timing()))
    (states, summary), timing = got
    assert np.array_equal(states, want[0]) and np.array_equal(summary, want[1])
    assert timing["play_launches"] >= 6, timing  # five launches for the first generation alone, then the replacements


@pytest.mark.parametrize("call", [dict(max_rounds=200), dict(max_rounds=200, target_score=2025), dict(max_rounds=200, target=37, max_attempts=37)],
                         ids=["clean", "target-2025", "no-replacements"])
def test_clean_case(eng, oracle, table, call):
    args = {**HARD, **call}
    want_states, want_summary = oracle.h2h_round_robin(table, **args)
    if call == dict(max_rounds=200):  # what the oracle gives here: 126 complete blocks without a safety-limit game, 6 with none completed
        flat = want_states.reshape(-1, 5)
        assert int(((flat[:, 1] == 37) & (flat[:, 2] == 0)).sum()) == 126 and int((flat[:, 1] == 0).sum()) == 6
    states, summary = eng.h2h_round_robin(table, **args)
    assert np.array_equal(states, want_states) and np.array_equal(summary, want_summary)


def test_ranges_concatenate_and_summaries_accumulate(eng, table, hard_ref):
    from farkle_ii_amd import round_robin as rr

    acc = np.zeros((12, 8), dtype=np.int64)
    parts = []
    for lo, hi in ((0, 20), (20, 66)):  # two adjacent ranges into one summary buffer
        states, out = eng.h2h_round_robin(table, pair_begin=lo, pair_end=hi, summary=acc, **HARD)
        assert out is acc and states.shape == (hi - lo, 2, 5)
        parts.append(states)
    assert np.array_equal(np.concatenate(parts), hard_ref[0]) and np.array_equal(acc, hard_ref[1])
    states, last = eng.h2h_round_robin(table, pair_begin=65, pair_end=66, **HARD)  # the last pair alone
    assert np.array_equal(states, hard_ref[0][65:]) and np.array_equal(last, rr.summary_from_states(12, hard_ref[0][65:], HARD["target"], 65, 66))
    before = acc.copy()
    for at in (0, 30, 66):  # an empty range touches nothing
        states, out = eng.h2h_round_robin(table, pair_begin=at, pair_end=at, summary=acc, **HARD)
        assert states.shape == (0, 2, 5) and out is acc and np.array_equal(acc, before)


def test_equals_the_explicit_block_path(eng, table, hard_ref):
    seats, pids, orders = stub.enumerate_blocks(table)
    explicit = eng.h2h_blocks(seats, HARD["root_seed"], pids, orders, HARD["target"], HARD["max_attempts"], chunk_games=HARD["max_attempts"],
                              max_rounds=HARD["max_rounds"])
    states, _ = eng.h2h_round_robin(table, **HARD)  # (after another table was resident)
    assert np.array_equal(states.reshape(-1, 5), explicit.astype(np.uint32)) and np.array_equal(states, hard_ref[0])


def test_smallest_tables_and_every_refusal(eng, oracle, table):
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    good = dict(root_seed=5, target=20, max_attempts=40, max_rounds=60)
    small = {n: stub.random_valid_table(n, 40 + n) for n in (2, 3)}
    want = {n: oracle.h2h_round_robin(small[n], **good) for n in (2, 3)}

    def still_good(n=3):
        states, summary = eng.h2h_round_robin(small[n], **good)
        assert np.array_equal(states, want[n][0]) and np.array_equal(summary, want[n][1])

    still_good(2)
    still_good(3)
    assert want[2][0].shape == (1, 2, 5) and want[3][0].shape == (3, 2, 5)
    bad_strategy = small[3].copy()
    bad_strategy["smart_five"][1], bad_strategy["smart_one"][1] = 0, 1
    refusals = [
        (dict(table=small[3][:1]), "a round robin needs at least two strategies, got 1"),
        (dict(pair_begin=2, pair_end=1), r"pair range \[2, 1\) is not inside the 3 pairs of 3 strategies"),
        (dict(pair_end=4), r"pair range \[0, 4\) is not inside the 3 pairs of 3 strategies"),
        (dict(target=0), r"target must be in \[1, max_attempts\] and max_attempts at most 2\^31 - 1"),
        (dict(target=41), r"target must be in \[1, max_attempts\]"),
        (dict(max_attempts=2**31), r"max_attempts at most 2\^31 - 1"),
        (dict(max_rounds=-1), r"max_rounds must be in \[0, 65535\]"),
        (dict(max_rounds=65536), r"max_rounds must be in \[0, 65535\]"),
        (dict(target_score=3_200_050), r"target_score 3200050: batched head-to-head plays with lean records \(totals up to 3200000 points\)"),
        (dict(table=bad_strategy), "strategy 1: smart_one requires smart_five"),
    ]
    for change, message in refusals:
        args = {**good, **change}
        tab = args.pop("table", small[3])
        summary = np.full((len(tab), 8), 7, dtype=np.int64)
        with pytest.raises(FarkleHipError, match=message) as err:
            eng.h2h_round_robin(tab, summary=summary, **args)
        assert err.value.code == FK_ERR_ARG and (summary == 7).all(), change
        still_good()
    with pytest.raises(ValueError, match="summary must be a C-contiguous int64 array"):
        eng.h2h_round_robin(small[3], summary=np.zeros((3, 8), dtype=np.int32), **good)
    for value in (0, 1, 33, (1 << 22) + 2):
        with pytest.raises(FarkleHipError, match="rr_window_blocks must be even and in"):
            eng.set_option("rr_window_blocks", value)
    assert eng.get_option("rr_window_blocks") == 1 << 22  # the default, untouched by the refused settings
    still_good()


def test_wide_table_of_one_attempt_blocks(eng, oracle):
    """300 strategies, 44 850 pairs, one attempt per block, eleven windows: conservation, the summary, and the oracle on a sample."""
    from farkle_ii_amd import round_robin as rr

    n, window = 300, 8192
    wide = stub.random_valid_table(n, 17)
    states, summary = _with_options(eng, {"rr_window_blocks": window}, lambda: eng.h2h_round_robin(wide, 29, 1, 1))
    flat = states.reshape(-1, 5).astype(np.int64)
    assert len(flat) == 2 * rr.pair_count(n) == 89_700
    assert (flat[:, 0] == 1).all() and (flat[:, 1] + flat[:, 2] == 1).all() and (flat[:, 3] + flat[:, 4] == flat[:, 1]).all()
    assert np.array_equal(summary, rr.summary_from_states(n, states, 1))
    assert summary[:, 0].tolist() == [n - 1] * n and int(summary[:, 2].sum()) == 2 * int(flat[:, 1].sum())
    seams = [b for w in range(window, len(flat), window) for b in (w - 1, w)]
    sample = sorted(set(range(0, len(flat), 601)) | set(seams) | {len(flat) - 1})
    pid = np.array([b // 2 for b in sample])
    i, j = rr.unrank(n, pid)
    orders = [b % 2 for b in sample]
    seats = np.stack([wide[[a, c]] if o == 0 else wide[[c, a]] for a, c, o in zip(i, j, orders)])
    want = oracle.h2h_blocks(seats, 29, pid.tolist(), orders, 1, 1, chunk_games=1)
    assert np.array_equal(flat[sample], want.astype(np.int64))
