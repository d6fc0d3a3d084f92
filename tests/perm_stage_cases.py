"""The permutation stage's cases and references (test helper, not a conftest): plain NumPy and Python ints.

The device rebuilds ``Generator.permutation`` of the stream ``(SHUFFLE_PERMUTATION, root, k, shuffle)`` with up to six kernels
(csrc/fk_kernels.h, csrc/fk_perm_wave.h).  Three references, each one step from the next and compared with it on the CPU
(``test_perm_stage_cpu.py``):

``numpy_perms``            NumPy's own ``Generator.permutation`` — what every generator-driven GPU result is compared with;
``literal_draws`` +        the accepted ``j`` of steps ``S - 1 .. 1`` restated from the raw 64-bit stream, and the plain swap loop over a
``literal_fisher_yates``   draw list — what the synthetic draw lists (which no generator produces) are compared with;
``wave_rounds``            a literal of the wave kernel's scheme (rounds of 128 words iterated from "none accepted" to the fixed point):
                           it only shows on the CPU which regimes a case reaches; no GPU result is compared with it.

The size lists hold ``(S, k, n_sh, shuffle0)``; ``k`` is the smallest divisor of ``S`` in [2, 128], or 1 where there is none.  The
synthetic lists are draw lists ``draws[n]`` = the ``j`` of step ``i = S - 1 - n``, each with ``draws[n] <= S - 1 - n`` by construction."""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np

from farkle_ii_amd.random import RandomPurpose, coordinate_rng, coordinate_seed_sequence

ROOT_SEED = 21
CSRC = Path(__file__).resolve().parent.parent / "farkle_ii_amd" / "csrc"
MODES = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (-1, -1))  # (perm_split, perm_draw_wave): six forced, one automatic


# ------------------------------------------------------------------------------------------------------------ the references
def numpy_perms(root: int, k: int, shuffle0: int, n_sh: int, S: int) -> np.ndarray:
    """int32 ``[n_sh][S]``: NumPy's ``Generator.permutation(S)`` of shuffles ``shuffle0 .. shuffle0 + n_sh - 1``."""
    out = np.empty((n_sh, S), dtype=np.int32)
    for s in range(n_sh):
        out[s] = coordinate_rng(RandomPurpose.SHUFFLE_PERMUTATION, root_seed=root, k=k, shuffle_index=shuffle0 + s).permutation(S)
    return out


def _words(root: int, k: int, shuffle: int):
    """The buffered 32-bit stream of a shuffle: of every 64-bit output the low half first, then the high half."""
    bits = np.random.PCG64DXSM(coordinate_seed_sequence(RandomPurpose.SHUFFLE_PERMUTATION, root_seed=root, k=k, shuffle_index=shuffle))
    while True:
        for o in bits.random_raw(256).tolist():
            yield o & 0xFFFFFFFF
            yield o >> 32


def literal_draws(root: int, k: int, shuffle: int, S: int) -> list[int]:
    """The accepted ``j`` of steps ``i = S - 1 .. 1``: a word masked with the bit length of the current ``i`` is accepted iff it is ``<= i``."""
    draws, i = [], S - 1
    words = _words(root, k, shuffle)
    while i >= 1:
        j = next(words) & ((1 << i.bit_length()) - 1)
        if j <= i:
            draws.append(j)
            i -= 1
    return draws


def literal_fisher_yates(S: int, draws) -> np.ndarray:
    """``a = arange(S); for i = S - 1 .. 1: swap(a[i], a[j_i])`` with ``j_i = draws[S - 1 - i]``."""
    a = list(range(S))
    assert len(draws) == max(S - 1, 0)
    for n, j in enumerate(draws):
        i = S - 1 - n
        a[i], a[j] = a[j], a[i]
    return np.array(a, dtype=np.int32)


def wave_rounds(root: int, k: int, shuffle: int, S: int) -> tuple[list[tuple[int, int, int]], list[int]]:
    """The wave kernel's scheme, literally: a round takes 128 words (lane L the words 2 L and 2 L + 1); every pass decides each word with
    the bound ``i`` less the words the PREVIOUS pass accepted in front of its lane (plus the lane's own low word of this pass), from "none
    accepted" until a pass changes nothing.  -> ``([(passes, bound at the round's begin, words accepted)] per round, the draws)``."""
    words = _words(root, k, shuffle)
    rounds, draws, i = [], [], S - 1
    while i >= 1:
        w = [next(words) for _ in range(128)]
        acc = [False] * 128
        passes = 0
        while True:
            passes += 1
            new, js, before = [False] * 128, [0] * 128, 0
            for lane in range(64):
                c = before
                for t in (2 * lane, 2 * lane + 1):
                    bound = max(i - c, 0)
                    js[t] = w[t] & ((1 << bound.bit_length()) - 1)
                    new[t] = bound >= 1 and js[t] <= bound
                    c += int(new[t])
                before += int(acc[2 * lane]) + int(acc[2 * lane + 1])
            if new == acc:
                break
            acc = new
        draws += [js[t] for t in range(128) if acc[t]]
        rounds.append((passes, i, sum(acc)))
        i -= sum(acc)
    return rounds, draws


def chain_free_literal(S: int, draws, skip_self_swap: bool = True) -> np.ndarray:
    """The chain-free kernel's scheme in plain Python (header of ``fk_perm_parallel_kernel``): the steps bucketed by target, ``U`` = the
    next step of the same bucket, ``F[p]`` = the bucket's first step beyond ``p`` (with ``skip_self_swap`` off: its first step, which is
    ``p`` itself when step ``p`` is a self-swap), the chains resolved by jumping.  It only shows on the CPU what the rule can change."""
    J = [0] * S
    for n, j in enumerate(draws):
        J[S - 1 - n] = j
    buckets = [[] for _ in range(S)]
    for i in range(1, S):
        buckets[J[i]].append(i)
    U, F = [None] * S, list(range(S))
    for p, steps in enumerate(buckets):
        for a, i in enumerate(steps):  # (ascending by construction)
            if a + 1 < len(steps):
                U[i] = steps[a + 1]
        beyond = [i for i in steps if (i > p if skip_self_swap else i >= p)]
        if beyond:
            F[p] = beyond[0]
    for _ in range(max(S.bit_length(), 1)):
        F = [F[f] for f in F]
    return np.array([F[0] if i == 0 else (F[U[i]] if U[i] is not None else J[i]) for i in range(S)], dtype=np.int32)


def wave_passes(root: int, k: int, shuffle: int, S: int) -> list[int]:
    """The number of passes of every round of ``wave_rounds`` (the last pass is the one that finds nothing changed)."""
    return [r[0] for r in wave_rounds(root, k, shuffle, S)[0]]


# --------------------------------------------------------------------------------------------- the sources' constants, restated
@lru_cache(maxsize=None)
def constants() -> dict:
    """Read out of the sources, so that a change there shows here."""
    hip = (CSRC / "farkle_hip.hip").read_text()
    kern = (CSRC / "fk_kernels.h").read_text()
    wave = (CSRC / "fk_perm_wave.h").read_text()

    def one(pattern: str, text: str):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]

    a, b = one(r"constexpr size_t LDS_LIMIT = (\d+) \* (\d+);", hip)
    per, less = one(r"bool perm_parallel_fits\(int32_t S\) \{ return \(size_t\)S \* (\d+) <= LDS_LIMIT - (\d+); \}", hip)
    assert one(r"uint32_t perm_slots\(int32_t S\) \{ return \(uint32_t\)std::max<size_t>\(1, std::min<size_t>\(PERM_BLOCK, LDS_LIMIT / \(\(size_t\)S \* (\d+)\)\)\); \}", hip) == "2"
    return {"LDS_LIMIT": int(a) * int(b), "PP_BYTES": int(per), "PP_STATIC": int(less),
            "PERM_BLOCK": int(one(r"constexpr int PERM_BLOCK = (\d+),", kern)), "PP_BLOCK": int(one(r"constexpr int PP_BLOCK = (\d+);", kern)),
            "DRAW_BLOCK": int(one(r"constexpr int DRAW_BLOCK = (\d+);", kern)),
            "WAVE_DRAW_BLOCK": int(one(r"constexpr int WAVE_DRAW_BLOCK = (\d+);", wave)),
            "WAVE_DRAW_MAX_SH": int(one(r"constexpr uint32_t WAVE_DRAW_MAX_SH = (\d+);", wave)),
            "JUMP_ROUNDS": int(one(r"for \(int round = 0; round < (\d+); \+\+round\)", kern))}


def perm_slots(S: int) -> int:
    c = constants()
    return max(1, min(c["PERM_BLOCK"], c["LDS_LIMIT"] // (2 * S)))


def parallel_fits(S: int) -> bool:
    c = constants()
    return S * c["PP_BYTES"] <= c["LDS_LIMIT"] - c["PP_STATIC"]


# --------------------------------------------------------------------------------------------------------------- the size lists
def smallest_k(S: int) -> int:
    return next((k for k in range(2, 129) if S % k == 0), 1)


def _entry(S: int, n_sh: int, shuffle0: int) -> tuple[int, int, int, int]:
    return (S, smallest_k(S), n_sh, shuffle0)


def _few(S: int) -> int:
    """3 to 40 shuffles up to S = 300, 3 to 8 beyond; spread by the size."""
    return 3 + (7 * S) % 38 if S <= 300 else 3 + S % 6


DENSE = tuple(_entry(S, _few(S), 13 * S) for S in range(2, 301))
DENSE_PARTS = tuple(DENSE[a:a + 50] for a in range(0, len(DENSE), 50))  # the same sizes, split so that a test stays short
BIT_LENGTHS = {b: tuple(_entry((1 << b) + d, _few((1 << b) + d), 1000) for d in (-1, 0, 1, 2)) for b in range(9, 16)}
LDS_SEAMS = {"slots_512_508": tuple(_entry(S, 8, 1000) for S in (160, 161)),
             "chain_free_last_and_first_beyond": tuple(_entry(S, 5, 1000) for S in (11628, 11629, 11630)),
             "slots_2_1": tuple(_entry(S, 5, 1000) for S in (40960, 40961))}
TOP = tuple(_entry(S, 3, 1000) for S in (65533, 65534, 65535))
COUNT_SIZES = (8, 96, 5160)


def shuffle_counts(S: int) -> tuple[int, ...]:
    return (1, 4, 5, 63, 64, 65, 128, 256, 257, perm_slots(S), perm_slots(S) + 1)


SHUFFLE_COUNTS = {S: tuple(_entry(S, n, 1000) for n in shuffle_counts(S)) for S in COUNT_SIZES}
DRAW_CHOICE_SEAM = ((8, 2, 32768, 1000), (8, 2, 32769, 1000))  # WAVE_DRAW_MAX_SH and one more, perm_draw_wave = -1
SHUFFLE0S = (0, 2**32 - 2, 2**32 + 5, 2**40 + 7, 2**63 - 300)
SHUFFLE0 = {s0: tuple(_entry(S, 12 if S <= 300 else 5, s0) for S in (9, 96, 1290, 5160)) for s0 in SHUFFLE0S}


def all_entries() -> list[tuple[int, int, int, int]]:
    out = list(DENSE) + list(TOP) + list(DRAW_CHOICE_SEAM)
    for group in (BIT_LENGTHS, LDS_SEAMS, SHUFFLE_COUNTS, SHUFFLE0):
        for entries in group.values():
            out += entries
    return out


def split_layouts(S: int) -> tuple[int, ...]:
    """The split layouts a forced split call of S strategies runs on: 1 = group-major (the swap chains), 2 = rows (the chain-free kernel)."""
    return (1, 2) if parallel_fits(S) else (1,)


# -------------------------------------------------------------------------------------------------------- the synthetic draw lists
SYNTH_SIZES = (2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 64, 65, 1024, 1025, 4097)
SYNTH_SEAM_SIZES = (11628, 11629)        # the chain-free kernel near its LDS limit: rotation, self-swap, halving, uniform
SYNTH_SEAM_KINDS = ("rotation", "self", "halving", "uniform")
ONE_BUCKET_CAP = 2049                    # path 2: a thread sorts a whole bucket by insertion, quadratic in its size


def _steps(S: int) -> range:
    return range(S - 1, 0, -1)           # i of draw n = S - 1 - n


SYNTH = {
    "self": lambda S: [i for i in _steps(S)],                                  # every step a self-swap: the identity
    "zero": lambda S: [0 for i in _steps(S)],                                  # one bucket holds every step
    "rotation": lambda S: [i - 1 for i in _steps(S)],                          # position 0's pointer chain has length S - 1
    "halving": lambda S: [i // 2 for i in _steps(S)],
    "const_1": lambda S: [min(i, 1) for i in _steps(S)],                       # a large bucket with its own self-swap inside
    "const_half": lambda S: [min(i, S // 2) for i in _steps(S)],
    "const_top": lambda S: [min(i, max(S - 2, 0)) for i in _steps(S)],
    "zero_self": lambda S: [0 if i % 2 else i for i in _steps(S)],             # alternating zero and self
    "uniform": lambda S: [int(v) for v in np.random.default_rng(S).integers(0, np.arange(S - 1, 0, -1) + 1)],
}
ONE_BUCKET_KINDS = ("zero", "const_1", "const_half", "const_top")  # the all-zero and the constant lists: capped on path 2


def synth_cases(path: int) -> list[tuple[str, int]]:
    """``(kind, S)`` of every synthetic list a path takes."""
    out = [(kind, S) for kind in SYNTH for S in SYNTH_SIZES if not (path == 2 and kind in ONE_BUCKET_KINDS and S > ONE_BUCKET_CAP)]
    if path == 2:
        out += [(kind, S) for kind in SYNTH_SEAM_KINDS for S in SYNTH_SEAM_SIZES]
    return out


@lru_cache(maxsize=None)
def synth_draws(kind: str, S: int) -> np.ndarray:
    d = np.array(SYNTH[kind](S), dtype=np.int64).reshape(S - 1)
    assert np.all(d >= 0) and np.all(d <= np.arange(S - 1, 0, -1)), (kind, S)
    d = d.astype(np.uint16)
    d.setflags(write=False)
    return d


@lru_cache(maxsize=None)
def synth_want(kind: str, S: int) -> np.ndarray:
    want = literal_fisher_yates(S, synth_draws(kind, S).tolist())
    want.setflags(write=False)
    return want
