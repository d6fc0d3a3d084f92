"""The references of ``test_perm_stage_gpu.py`` are NumPy's, and its cases reach the regimes they are there for — shown here without
a GPU: the literal draws and swap loop of ``perm_stage_cases.py`` give ``Generator.permutation`` for every entry of every size list;
the lists hold every draw-group tail for both split layouts and sit on the seams the sources' constants put there; the wave scheme's
literal takes one, two and three-pass rounds on listed cases; every synthetic draw list obeys ``j <= i``."""
from __future__ import annotations

import numpy as np
import pytest

import perm_stage_cases as pc

ROOT = pc.ROOT_SEED


def _sample(S: int, n_sh: int) -> list[int]:
    """Every shuffle of a small entry; of a large one the first, the middle and the last, and the two beside a multiple of 2^15."""
    if n_sh * S <= 20_000:
        return list(range(n_sh))
    return sorted({0, n_sh // 2, n_sh - 1} | {s for s in (32767, 32768) if s < n_sh})


LISTS = {**{f"dense{n}": part for n, part in enumerate(pc.DENSE_PARTS)}, **{f"bits{b}": e for b, e in pc.BIT_LENGTHS.items()},
         **pc.LDS_SEAMS, "top": pc.TOP, **{f"counts{S}": e for S, e in pc.SHUFFLE_COUNTS.items()}, "draw_choice": pc.DRAW_CHOICE_SEAM,
         **{f"shuffle0_{s0:#x}": e for s0, e in pc.SHUFFLE0.items()}}


def test_the_parametrised_lists_are_all_the_entries():
    assert sorted(e for entries in LISTS.values() for e in entries) == sorted(pc.all_entries())
    assert [S for S, _, _, _ in pc.DENSE] == list(range(2, 301))
    for S, k, n_sh, s0 in pc.all_entries():
        assert S % k == 0 and 1 <= k <= 128 and (k > 1 or all(S % d for d in range(2, 129))) and n_sh >= 1 and s0 + n_sh <= 2**64
        if (S, k, n_sh, s0) not in pc.DRAW_CHOICE_SEAM and all((S, k, n_sh, s0) not in e for e in pc.SHUFFLE_COUNTS.values()):
            assert 3 <= n_sh <= (40 if S <= 300 else 8)


@pytest.mark.parametrize("name", list(LISTS))
def test_literal_draws_and_swap_loop_are_numpys_permutation(name):
    for S, k, n_sh, s0 in LISTS[name]:
        for s in _sample(S, n_sh):
            draws = pc.literal_draws(ROOT, k, s0 + s, S)
            assert len(draws) == S - 1 and all(j <= S - 1 - n for n, j in enumerate(draws))
            assert np.array_equal(pc.literal_fisher_yates(S, draws), pc.numpy_perms(ROOT, k, s0 + s, 1, S)[0]), (S, k, s0 + s)


def test_numpy_perms_is_the_oracles_permutation_at_three_points():
    import pyoracle as po

    for S, k, shuffle in ((9, 3, 1000), (15, 3, 2**40 + 7), (11629, 29, 5)):
        assert np.array_equal(pc.numpy_perms(ROOT, k, shuffle, 1, S)[0], po.permutation(po.coord(101, ROOT, k=k, shuffle_index=shuffle), S))


def test_every_tail_occurs_for_both_split_layouts():
    tails = {1: set(), 2: set()}
    for S, _, _, _ in pc.all_entries():
        for layout in pc.split_layouts(S):
            tails[layout].add((S - 1) & 7)
    assert tails[1] == tails[2] == set(range(8))
    # ... and beyond the dense list too: a full last group (tail 0) and even tails on tables of thousands of strategies
    large = {layout: {(S - 1) & 7 for S, _, _, _ in pc.all_entries() if S > 1024 and layout in pc.split_layouts(S)} for layout in (1, 2)}
    assert {0, 4, 6} <= large[1] and {0, 4, 6} <= large[2]
    for path in (1, 2):
        assert {(S - 1) & 7 for _, S in pc.synth_cases(path)} == set(range(8))


def test_the_seams_are_where_the_sources_put_them():
    c = pc.constants()
    assert 11629 * c["PP_BYTES"] <= c["LDS_LIMIT"] - c["PP_STATIC"] < 11630 * c["PP_BYTES"]
    assert [pc.parallel_fits(S) for S, _, _, _ in pc.LDS_SEAMS["chain_free_last_and_first_beyond"]] == [True, True, False]
    assert [pc.perm_slots(S) for S in (160, 161, 40960, 40961)] == [512, 508, 2, 1]
    assert [S for S, _, _, _ in pc.LDS_SEAMS["slots_512_508"] + pc.LDS_SEAMS["slots_2_1"]] == [160, 161, 40960, 40961]
    # the exclusive scan of the chain-free kernel: 12 table entries per thread at the last size that fits, and start[] in u16 near its top
    assert -(-11629 // c["PP_BLOCK"]) == 12 and 11629 < 0xFFFF
    assert max(S for S, _, _, _ in pc.all_entries()) == 65535 and (65535 - 1) & 7 == 6  # the largest index 0xfffe, beside PP_NONE
    # the strides of a launch: a wave-draw workgroup's four shuffles, n_sh_pad's 64, DRAW_BLOCK, a block's slots, the draw choice
    assert c["WAVE_DRAW_BLOCK"] // 64 == 4 and c["DRAW_BLOCK"] == 256 and c["WAVE_DRAW_MAX_SH"] == 32768
    for S in pc.COUNT_SIZES:
        counts = pc.shuffle_counts(S)
        assert {1, 4, 5, 63, 64, 65, 128, c["DRAW_BLOCK"], c["DRAW_BLOCK"] + 1, pc.perm_slots(S), pc.perm_slots(S) + 1} == set(counts)
    assert [n for _, _, n, _ in pc.DRAW_CHOICE_SEAM] == [c["WAVE_DRAW_MAX_SH"], c["WAVE_DRAW_MAX_SH"] + 1]
    assert [pc.perm_slots(S) for S in pc.COUNT_SIZES] == [512, 512, 15]
    # the pointer jumping's round bound covers the longest chain of the largest table that fits, and one round that finds no change
    assert (11629 - 1).bit_length() + 1 <= c["JUMP_ROUNDS"]
    # every shuffle0 entry's count crosses the 2^32 carry where its start lies below it
    for s0, entries in pc.SHUFFLE0.items():
        for _, _, n_sh, _ in entries:
            assert not (2**32 - 64 < s0 < 2**32) or s0 + n_sh > 2**32
    assert any(s0 >> 32 for s0 in pc.SHUFFLE0S) and any(s0 >> 62 for s0 in pc.SHUFFLE0S)


# (S, k, shuffle) of listed entries whose rounds the wave scheme's literal is run on
WAVE_CASES = [(S, k, s0 + s) for S, k, n_sh, s0 in (pc.DENSE[64 - 2], pc.DENSE[300 - 2], pc.SHUFFLE_COUNTS[5160][1], pc.SHUFFLE0[2**40 + 7][2], pc.TOP[2])
              for s in range(min(n_sh, 3))]


def test_wave_scheme_literal_reaches_every_regime_and_gives_the_sequential_draws():
    rounds = {}
    for S, k, shuffle in WAVE_CASES:
        rounds[S, k, shuffle], draws = pc.wave_rounds(ROOT, k, shuffle, S)
        assert draws == pc.literal_draws(ROOT, k, shuffle, S), (S, k, shuffle)  # the fixed point is the sequential result
        assert pc.wave_passes(ROOT, k, shuffle, S) == [r[0] for r in rounds[S, k, shuffle]]
    every = [r for rs in rounds.values() for r in rs]
    passes = [r[0] for r in every]
    print("rounds by passes:", {p: passes.count(p) for p in sorted(set(passes))})
    assert max(passes) >= 3                  # a round whose first estimate was wrong: a third pass
    assert 2 in passes                       # a round whose first estimate stood: only the pass that finds nothing changed
    assert any(S <= 64 and len(rs) == 1 for (S, _, _), rs in rounds.items())  # a shuffle that ends inside its first round
    # a round in which the bound passes a power of two, so that words of one round are masked with two bit lengths (a round that
    # rejects every word cannot be had: a word is rejected with probability below one half)
    crossing = [(p, i, a) for p, i, a in every if i.bit_length() != max(i - a + 1, 1).bit_length()]
    assert crossing and any(p >= 3 for p, _, _ in crossing)
    assert all(a >= 1 for _, _, a in every) and min(passes) >= 2


def test_chain_free_scheme_on_every_draw_list_of_small_tables_and_what_its_self_swap_rule_changes():
    """Bucket sort + pointer jumping gives the swap loop's result for every draw list of 2 to 7 strategies and for the synthetic lists.
    It does so with and without the rule that a bucket's self-swap (step p targeting p) is not p's next step: ``F[p]`` of a
    self-swapping p is read by nobody (a chain reaches p only through a step p that targets a position below p, and the rest of the
    bucket hangs on ``U``), so no result can show that rule: ``i > p`` against ``i >= p`` in the kernel is not a fault a test can find."""
    from itertools import product

    lists = [list(js) for S in range(2, 8) for js in product(*[range(i + 1) for i in range(S - 1, 0, -1)])]
    lists += [pc.synth_draws(kind, S).tolist() for kind in pc.SYNTH for S in pc.SYNTH_SIZES if S <= 65]
    assert len(lists) > 5000
    for draws in lists:
        S = len(draws) + 1
        want = pc.literal_fisher_yates(S, draws)
        assert np.array_equal(pc.chain_free_literal(S, draws), want), draws
        assert np.array_equal(pc.chain_free_literal(S, draws, skip_self_swap=False), want), draws


@pytest.mark.parametrize("path", [1, 2])
def test_synthetic_lists_obey_their_bounds(path):
    cases = pc.synth_cases(path)
    assert len(set(cases)) == len(cases)
    for kind, S in cases:
        d = pc.synth_draws(kind, S)
        assert d.dtype == np.uint16 and d.shape == (S - 1,) and np.all(d.astype(np.int64) <= np.arange(S - 1, 0, -1)), (kind, S)
        assert path == 1 or pc.parallel_fits(S)
    sizes = {S for _, S in cases}
    assert set(pc.SYNTH_SIZES) <= sizes and (set(pc.SYNTH_SEAM_SIZES) <= sizes) == (path == 2)
    capped = {kind for kind in pc.SYNTH if (kind, 4097) not in cases}
    assert capped == (set(pc.ONE_BUCKET_KINDS) if path == 2 else set())
    assert max(S for kind, S in cases if kind in pc.ONE_BUCKET_KINDS) == (1025 if path == 2 else 4097) and pc.ONE_BUCKET_CAP == 2049


def test_synthetic_lists_are_what_their_names_say():
    for S in pc.SYNTH_SIZES + pc.SYNTH_SEAM_SIZES:
        assert np.array_equal(pc.synth_want("rotation", S), np.r_[S - 1, np.arange(S - 1)])
        assert np.array_equal(pc.synth_want("self", S), np.arange(S))
        # the rotation's chain of position 0 runs through every step: ceil(log2 S) jumping rounds
        assert pc.synth_draws("rotation", S).tolist() == list(range(S - 2, -1, -1))
    for S in pc.SYNTH_SIZES:
        assert not pc.synth_draws("zero", S).any()
        d = pc.synth_draws("const_1", S).astype(int)
        assert d[-1] == 1 and (S < 3 or np.all(d[:-1] == 1))  # bucket 1 holds every step, its own self-swap (step 1) among them
        for kind in pc.SYNTH:
            assert sorted(pc.synth_want(kind, S).tolist()) == list(range(S)), (kind, S)
    # a chain of S - 1 hops takes ceil(log2(S - 1)) rounds: 12 at 4 097, 14 at the seam sizes (where a lower round bound would show)
    assert (4097 - 2).bit_length() == 12 and all((S - 2).bit_length() == 14 for S in pc.SYNTH_SEAM_SIZES)
