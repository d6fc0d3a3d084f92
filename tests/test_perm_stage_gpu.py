"""The permutation stage on the GPU against NumPy itself, at every draw-group tail, table-size edge and shuffle-count stride, and its
two draw consumers against the plain swap loop on draw lists no generator produces (``perm_stage_cases.py``;
``test_perm_stage_cpu.py`` pins those references to NumPy and shows which regimes the cases reach).

Generator-driven: ``Engine.tournament(..., want_perms=True, max_rounds=0)`` — every game stops at once, so a call is all permutation
stage — under ``perm_split`` 0, 1, 2 with ``perm_draw_wave`` 0 and 1, and once with both automatic.  The permutations are NumPy's
``Generator.permutation``; the tally says that every strategy sat once per shuffle in a game that ran into the round limit and
nothing else (attempted = safety = the shuffles of the batch, every other column zero).

Synthetic: ``Engine.debug_perm_from_draws`` hands a draw list to ``fk_perm_apply_kernel`` (path 1) or to
``fk_perm_parallel_kernel`` + ``fk_perm_block_kernel`` (path 2) as a tournament chunk launches them."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import kernel_instances as ki
import perm_stage_cases as pc

pytestmark = pytest.mark.gpu
ROOT = pc.ROOT_SEED
ATTEMPTED, SAFETY = 1, 3  # tally columns (include/farkle_hip.h: wins, attempted, completed, safety, 11 sums, 11 square sums)


@pytest.fixture(scope="module")
def eng():
    from farkle_ii_amd.backend import Engine

    e = Engine(0)
    yield e
    e.close()


@lru_cache(maxsize=None)
def _table(S: int) -> np.ndarray:
    t = ki._random_legal(S, S)
    t["strategy_id"] = np.arange(S)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def _want(S: int, k: int, n_sh: int, shuffle0: int) -> np.ndarray:
    want = pc.numpy_perms(ROOT, k, shuffle0, n_sh, S)
    want.setflags(write=False)
    return want


def _check_call(eng, entry, mode) -> None:
    S, k, n_sh, s0 = entry
    got = eng.tournament(_table(S), k, ROOT, s0, s0 + n_sh, want_perms=True, max_rounds=0)
    want = _want(*entry)
    assert np.array_equal(got["perms"], want), (entry, mode, np.argwhere(got["perms"] != want)[:4].tolist())
    tally = got["tally"]
    assert tally.shape == (1, S, 26)
    # one safety-limit exposure per strategy and shuffle, and nothing else (attempted = completed + safety)
    assert np.all(tally[0, :, SAFETY] == n_sh) and np.all(tally[0, :, ATTEMPTED] == n_sh), (entry, mode)
    assert not np.delete(tally[0], (ATTEMPTED, SAFETY), axis=1).any(), (entry, mode)


def _check_entries(eng, entries, modes=pc.MODES) -> None:
    try:
        for entry in entries:
            for split, wave in modes:
                eng.set_option("perm_split", split)
                eng.set_option("perm_draw_wave", wave)
                _check_call(eng, entry, (split, wave))
    finally:
        eng.set_option("perm_split", -1)
        eng.set_option("perm_draw_wave", -1)


# ------------------------------------------------------------------------------------------------------------- generator-driven
@pytest.mark.parametrize("part", range(len(pc.DENSE_PARTS)))
def test_dense_sizes_every_tail_on_every_path(eng, part):
    """Every S from 2 to 300 (fifty per case): all eight tails of the last draw group, odd tables among them, on all seven paths."""
    _check_entries(eng, pc.DENSE_PARTS[part])


@pytest.mark.parametrize("b", list(pc.BIT_LENGTHS))
def test_sizes_around_a_power_of_two(eng, b):
    """2^b - 1 .. 2^b + 2: the first draws' masks change bit length, the last group is partial (tails 6, 7, 1) or full (2^b + 1)."""
    _check_entries(eng, pc.BIT_LENGTHS[b])


@pytest.mark.parametrize("seam", list(pc.LDS_SEAMS))
def test_lds_seams(eng, seam):
    """512 against 508 and two against one shuffles per block; 11 628 / 11 629 fill the chain-free kernel's LDS (twelve table entries per
    thread in its scan), 11 630 does not fit it: ``perm_split`` 2 falls back to the swap chains there and still gives NumPy's result."""
    _check_entries(eng, pc.LDS_SEAMS[seam])


@pytest.mark.parametrize("entry", pc.TOP, ids=lambda e: str(e[0]))
def test_largest_tables(eng, entry):
    """65 533 .. 65 535: the last is the largest table the entry takes, its largest index 0xfffe, its last draw group six draws."""
    _check_entries(eng, [entry])


@pytest.mark.parametrize("S", pc.COUNT_SIZES)
def test_shuffle_counts_at_the_strides(eng, S):
    """1 shuffle; 4 | 5 (a wave-draw workgroup's four); 63 .. 65 and 128 (the group-major layout pads to 64); 256 | 257 (a draw block);
    a permutation block's slots and one more."""
    _check_entries(eng, pc.SHUFFLE_COUNTS[S])


def test_draw_choice_seam(eng):
    """32 768 | 32 769 shuffles in one call: the automatic choice between a wave and a thread per shuffle flips.  Equal results only
    (nothing shows which kernel ran)."""
    assert _want(*pc.DRAW_CHOICE_SEAM[0]).shape == (32768, 8)
    _check_entries(eng, pc.DRAW_CHOICE_SEAM, modes=((1, -1), (2, -1)))


@pytest.mark.parametrize("shuffle0", pc.SHUFFLE0S, ids=hex)
def test_shuffle_index_high_word(eng, shuffle0):
    """Shuffle indices with a high word, and ranges across the 2^32 carry, on the split and wave paths (tables of 9 to 5 160)."""
    _check_entries(eng, pc.SHUFFLE0[shuffle0])


# -------------------------------------------------------------------------------------------------------------------- synthetic
SMALL = (96, 2, 7, 1000)  # the generator-driven call behind every synthetic one: buffers only grow, it must not see what they held


def _synth_sizes(path: int) -> list[int]:
    return sorted({S for _, S in pc.synth_cases(path)})


@pytest.mark.parametrize("path,S", [(path, S) for path in (1, 2) for S in _synth_sizes(path)])
def test_draw_consumers_on_synthetic_lists(eng, path, S):
    """Every list of the size in one call, three times over (so that the call fills more than one block at the large sizes): each row
    is the plain swap loop's result.  Rotation: ceil(log2(S - 1)) pointer-jumping rounds; zero / const: one bucket of every step, a
    self-swap inside it; self: no swap at all."""
    kinds = [kind for kind, size in pc.synth_cases(path) if size == S] * 3
    draws = np.stack([pc.synth_draws(kind, S) for kind in kinds])
    got = eng.debug_perm_from_draws(S, draws, path)
    assert got.shape == (len(kinds), S) and got.dtype == np.int32
    for row, kind in enumerate(kinds):
        want = pc.synth_want(kind, S)
        assert np.array_equal(got[row], want), (path, S, kind, row, np.argwhere(got[row] != want)[:4].tolist())
    _check_entries(eng, [SMALL], modes=((path, -1), (-1, -1)))


def test_debug_entry_refusals(eng):
    """Every refusal is FK_ERR_ARG, leaves the result array as it was, and the next good call is right.  An out-of-range draw is found
    on the host: nothing is launched."""
    from farkle_ii_amd.backend import FK_ERR_ARG, FarkleHipError

    def refused(S, n_sh, draws, path):
        out = np.full((max(n_sh, 1), max(S, 1)), -7, dtype=np.int32)
        with pytest.raises(FarkleHipError) as err:
            eng.debug_perm_from_draws(S, draws, path, out=out, n_sh=n_sh)
        assert err.value.code == FK_ERR_ARG, (S, n_sh, path, err.value)
        assert np.all(out == -7), (S, n_sh, path)

    good = pc.synth_draws("uniform", 9)
    for path in (1, 2):
        refused(0, 1, np.zeros(1, np.uint16), path)
        refused(-1, 1, np.zeros(1, np.uint16), path)
        refused(65536, 1, np.zeros((1, 65535), np.uint16), path)
        refused(9, 0, good, path)
        refused(9, -1, good, path)
        for row, n, bound in ((0, 0, 8), (0, 7, 1), (1, 3, 5), (2, 7, 1)):  # first and last draw, another shuffle; one beyond the bound, and 0xffff
            for value in (bound + 1, 0xFFFF):
                draws = np.stack([good] * 3)
                draws[row, n] = value
                refused(9, 3, draws, path)
        assert np.array_equal(eng.debug_perm_from_draws(9, np.stack([good] * 3), path), np.stack([pc.synth_want("uniform", 9)] * 3))
    refused(9, 1, good, 0)
    refused(9, 1, good, 3)
    beyond = pc.LDS_SEAMS["chain_free_last_and_first_beyond"][2][0]
    assert not pc.parallel_fits(beyond) and pc.parallel_fits(beyond - 1)
    refused(beyond, 1, np.zeros((1, beyond - 1), np.uint16), 2)  # (all zero: a good list; on path 1 it is accepted)
    assert np.array_equal(eng.debug_perm_from_draws(beyond, np.arange(beyond - 1, 0, -1).astype(np.uint16)[None], 1)[0], np.arange(beyond))
    for path in (1, 2):  # a table of one strategy has no draw
        assert np.array_equal(eng.debug_perm_from_draws(1, np.zeros((2, 0), np.uint16), path, n_sh=2), np.zeros((2, 1), np.int32))
    _check_entries(eng, [SMALL], modes=((1, -1), (2, -1), (-1, -1)))
