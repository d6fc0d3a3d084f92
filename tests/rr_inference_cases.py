"""The families the round-robin inference tests run on, and the comparison of a device result with the host statement.

``synthetic_family``: 12 strategies (66 pairs), two roots, target 2 191 of at most 2 300 attempts; block states built by hand so that
the family holds every case the inference distinguishes (see ``SPECIAL``).  ``random_family``: n strategies, binomial counts."""
from __future__ import annotations

import numpy as np

import rr_inference_literal as lit

N = 12
TARGET, MAX_ATTEMPTS = 2191, 2300
PARAMS = dict(family_alpha=0.02, practical_delta=0.03, min_candidate_completion_rate=0.99)
DELTA_EQUIVALENCE = 0.03
WEAK = 11          # the strategy below the completion threshold: 60 safety-limit games in every one of its blocks
SHORT = (8, 9)     # the pair with a block one game short of its target (root 1, order 0)
# (i, j) -> (A's wins in order 0, B's wins in order 1) per root; every other pair draws its rates from EFFECTS
SPECIAL = {
    (0, 1): (1150, 1050), (0, 2): (1150, 1050), (1, 2): (1150, 1050), (3, 4): (1150, 1050), (5, 6): (1150, 1050),  # identical: p ties
    (0, 3): (2191, 0), (1, 4): (2191, 0), (2, 5): (2191, 0),   # 2 191 : 0 in both orders: |z| ~ 66, p exactly 0.0
    (0, 4): (1100, 1100), (1, 5): (987, 987),                  # equal counts in both orders: z = 0, p = 1, symmetric interval
    (2, 6): (0, 1000), (3, 7): (2191, 1200),                   # 0 / n and n / n in one order
}
# half-differences of the drawn pairs: practical dominance both ways, statistical-only both ways, equivalent, unresolved
EFFECTS = (0.09, -0.085, 0.035, -0.036, 0.004, -0.006, 0.0235, -0.0265, 0.06, 0.0, 0.013, -0.015)


def _pairs(n: int):
    from farkle_ii_amd import round_robin as rr

    _, i, j = rr.pair_ids(n)
    return [(int(a), int(b)) for a, b in zip(i, j)]


def synthetic_family() -> tuple[int, list[np.ndarray], int, int]:
    """``(n, [states of root 0, states of root 1], target, max_attempts)``, states uint32 ``[66, 2, 5]``."""
    rng = np.random.default_rng(4382)
    pairs = _pairs(N)
    roots = [np.zeros((len(pairs), 2, 5), dtype=np.uint32) for _ in range(2)]
    for p, (i, j) in enumerate(pairs):
        for r, st in enumerate(roots):
            if (i, j) in SPECIAL:
                x_ab, x_ba = SPECIAL[(i, j)]
            else:
                e = EFFECTS[p % len(EFFECTS)]
                x_ab, x_ba = (int(v) for v in rng.binomial(TARGET, (0.5 + e, 0.5 - e)))
            safety = 60 if WEAK in (i, j) else 0
            for order, wins1 in ((0, x_ab), (1, x_ba)):
                st[p, order] = (TARGET + safety, TARGET, safety, wins1, TARGET - wins1)
            if (i, j) == SHORT and r == 1:  # the attempt cap reached one completed game short of the target
                st[p, 0] = (MAX_ATTEMPTS, TARGET - 1, MAX_ATTEMPTS - (TARGET - 1), 1100, TARGET - 1 - 1100)
    return N, roots, TARGET, MAX_ATTEMPTS


def random_family(n: int = 300, games: int = 200, seed: int = 7) -> tuple[int, list[np.ndarray], int, int]:
    """One root of binomial counts at ``games`` games per block: rates spread around one half, a few blocks short of their target."""
    rng = np.random.default_rng(seed)
    n_pairs = n * (n - 1) // 2
    skill = rng.normal(0.0, 0.08, size=n)
    pairs = np.array(_pairs(n))
    gap = np.clip(skill[pairs[:, 0]] - skill[pairs[:, 1]], -0.45, 0.45)
    st = np.zeros((n_pairs, 2, 5), dtype=np.uint32)
    x_ab, x_ba = rng.binomial(games, 0.5 + gap), rng.binomial(games, 0.5 - gap)
    for order, wins1 in ((0, x_ab), (1, x_ba)):
        st[:, order] = np.stack([np.full(n_pairs, games), np.full(n_pairs, games), np.zeros(n_pairs), wins1, games - wins1], axis=1)
    short = rng.choice(n_pairs, size=7, replace=False)  # blocks that used every attempt without reaching the target
    st[short, 1] = (2 * games, games - 3, games + 3, 90, games - 93)
    return n, [st], games, 2 * games


def assert_margins(host: dict, practical_delta: float, delta_equivalence: float | None, family_alpha: float) -> None:
    """The families are chosen so that no decision hangs on the last digits: no simultaneous bound within 1e-9 of a threshold, no
    adjusted p within a factor 1 +- 1e-9 of alpha.  With that, a device result inside the bounds' tolerance has the host's classes."""
    rows = host["rows"]
    tested = (rows["flags"] & 1) != 0
    for edge in (practical_delta, -practical_delta) + (() if delta_equivalence is None else (delta_equivalence, -delta_equivalence)):
        for name in ("simultaneous_d_low", "simultaneous_d_high"):
            assert np.abs(rows[name][tested] - edge).min() > 1e-9, (name, edge)
    adjusted = rows["holm_adjusted_p"][tested]
    assert (np.abs(adjusted / family_alpha - 1.0) > 1e-9).all()


EXACT_FIELDS = ("pair_id", "strategy_a", "strategy_b", "games_attempted", "games_completed", "games_safety_limit", "n_completed_required",
                "n_ab", "n_ba", "seat1_a_wins_ab", "seat1_b_wins_ba", "seat2_a_wins_ba", "balanced_a_wins", "flags", "decision_class",
                "completion_game_rate", "q_ab", "q_ba", "raw_order_rate_difference", "d_ab", "score_null_proportion", "score_z",
                "balanced_a_win_rate")
BOUND_FIELDS = ("ordinary_d_low", "ordinary_d_high", "simultaneous_d_low", "simultaneous_d_high")


def p_value_bound(z: np.ndarray) -> np.ndarray:
    """Relative distance allowed between the device's erfc(|z| / sqrt 2) and 2 norm.sf(|z|): (8 + z^2) 2^-52 — z^2 is the
    conditioning of exp(-z^2 / 2) on a half-ulp change of its argument, which every library pays; the 8 is for the library's
    own polynomial."""
    return (8.0 + z * z) * 2.0**-52


def compare(dev: dict, host: dict) -> None:
    """A device result against the host statement of the same counts and parameters."""
    from scipy.stats import norm

    got, want = dev["rows"], host["rows"]
    assert got.shape == want.shape
    for name in EXACT_FIELDS:  # bit-equal (NaN where a pair has no test, in both)
        assert got[name].tobytes() == want[name].tobytes(), name
    assert not got["pad"].any()
    tested = (want["flags"] & 1) != 0
    for name in BOUND_FIELDS + ("score_p_value", "holm_adjusted_p"):
        assert np.array_equal(np.isnan(got[name]), ~tested), name
    for name in BOUND_FIELDS:  # the halved bounds: half of 2.5e-12
        assert np.abs(got[name][tested] - want[name][tested]).max(initial=0.0) <= 0.5 * lit.BOUND_TOL, name
    # p against 2 norm.sf(|z|) at the bit-equal z
    z = np.abs(want["score_z"][tested])
    p_ref, p_dev = 2.0 * norm.sf(z), got["score_p_value"][tested]
    normal = p_ref >= 2.3e-308
    assert (np.abs(p_dev[normal] - p_ref[normal]) <= p_value_bound(z[normal]) * p_ref[normal]).all()
    assert (p_dev[z >= 39.0] == 0.0).all()
    # Holm is exact as a function of the device's own p
    adjusted, place = lit.holm(np.where(tested, got["score_p_value"], 1.0))
    assert got["holm_adjusted_p"][tested].tobytes() == adjusted[tested].tobytes()
    assert np.array_equal(got["holm_order"], np.where(tested, place, 0))
    assert np.array_equal(dev["class_counts"], host["class_counts"])
    assert np.array_equal(dev["strategies"], host["strategies"])
