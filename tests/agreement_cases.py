"""The families the method-agreement tests run on: decision classes of every pair of a finalist table and a candidate membership.

A case is a dictionary: ``n`` and ``ids`` (the finalists' strategy ids, ascending: the table's rows), ``cls`` (uint8 per pair in
pair-id order), ``membership`` (a pandas frame in the layout of the reference's ``candidate_family.parquet``: one row per strategy of
the scored population, ranks as float64 with NaN for null — what reading its Int64 columns gives), ``family_hash``, ``root_summary``
(the twelve counts of ``fk_rr_root_diagnostics``, of which ``rr_root_diagnostics.stability_summary`` reads the first four) and
``execution_scope``.  ``CASES`` maps a name to a builder; ``all_cases()`` builds each once."""
from __future__ import annotations

import functools

import numpy as np

FAMILY_HASH = "agreement-test-family"
FLAGS = ("initial_win_rate_contribution", "initial_trueskill_contribution", "final_win_rate_contribution", "final_trueskill_contribution",
         "configured_control", "mandatory_diagnostic")


def build(n: int, population: int, seed: int, *, cls=None, classes=tuple(range(7)), win_null=(), ts_null=(), ts_absent: bool = False, tied: bool = False,
          available: int | None = None, scope: str = "root_pair") -> dict:
    """``n`` finalists drawn from a scored population of ``population`` strategies (ids 8, 9, ..).  ``cls``: the classes, default
    seeded draws from ``classes``.  ``win_null`` / ``ts_null``: finalist rows (table order) without that method's rank; ``ts_absent``:
    nobody has a TrueSkill rank; ``tied``: ranks repeat inside a method.  ``available``: pairs with a root agreement (default: all
    but a few)."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    n_pairs = n * (n - 1) // 2
    everyone = 8 + np.arange(population, dtype=np.int64)
    ids = np.sort(rng.choice(everyone, size=n, replace=False))
    if cls is None:
        cls = np.asarray(classes, dtype=np.uint8)[rng.integers(0, len(classes), size=n_pairs)]
    cls = np.asarray(cls, dtype=np.uint8)
    assert len(cls) == n_pairs
    if tied:
        win = rng.integers(1, max(2, population // 3) + 1, size=population).astype(np.float64)
        ts = rng.integers(1, max(2, population // 2) + 1, size=population).astype(np.float64)
    else:
        win = (1 + rng.permutation(population)).astype(np.float64)
        # correlated with the win-rate order, not equal to it
        ts = (1 + np.argsort(np.argsort(win + rng.normal(0.0, max(1.0, population / 6.0), size=population)))).astype(np.float64)
    row_of = {int(s): r for r, s in enumerate(everyone)}
    win[[row_of[int(ids[k])] for k in win_null]] = np.nan
    ts[[row_of[int(ids[k])] for k in ts_null]] = np.nan
    if ts_absent:
        ts[:] = np.nan
    if population > n + 4:  # a few of the others lack a rank too
        others = np.setdiff1d(np.arange(population), [row_of[int(s)] for s in ids])
        win[others[0]] = np.nan
        ts[others[1]] = np.nan
    final = np.isin(everyone, ids)
    flags = {name: rng.random(population) < 0.4 for name in FLAGS}
    for name in ("final_win_rate_contribution", "final_trueskill_contribution"):
        flags[name] &= final
    frame = pd.DataFrame({
        "strategy": pd.array(everyone, dtype="Int32"), "win_rate_rank": win, "trueskill_rank": ts,
        "scored_by_both_methods": ~np.isnan(win) & ~np.isnan(ts),
        "initial_win_rate_contribution": flags["initial_win_rate_contribution"], "initial_trueskill_contribution": flags["initial_trueskill_contribution"],
        "initial_shared_contribution": flags["initial_win_rate_contribution"] & flags["initial_trueskill_contribution"],
        "configured_control": flags["configured_control"], "mandatory_diagnostic": flags["mandatory_diagnostic"],
        "final_win_rate_contribution": flags["final_win_rate_contribution"], "final_trueskill_contribution": flags["final_trueskill_contribution"],
        "final_shared_contribution": flags["final_win_rate_contribution"] & flags["final_trueskill_contribution"],
        "final_family": final, "family_hash": FAMILY_HASH,
    })
    available = max(n_pairs - 3, 0) if available is None else int(available)
    root_summary = np.zeros(12, dtype=np.int64)
    root_summary[:4] = (n_pairs, available, int(rng.integers(0, available + 1)), int(rng.integers(0, available + 1)))
    return {"n": n, "ids": ids, "cls": cls, "membership": frame, "family_hash": FAMILY_HASH, "root_summary": root_summary, "execution_scope": scope}


CASES = {
    "two": lambda: build(2, 2, 1, available=1),
    "every_class": lambda: build(8, 12, 2, cls=np.arange(28) % 7),
    "null_ranks": lambda: build(7, 11, 3, win_null=(1, 4), ts_null=(2, 4)),  # row 4 lacks both
    "one_method_absent": lambda: build(6, 10, 4, ts_absent=True, available=0, scope="single_root"),
    "tied_ranks": lambda: build(9, 14, 5, tied=True),
    "no_directional": lambda: build(6, 9, 6, classes=(4, 5, 6)),
    "population_larger": lambda: build(9, 40, 7),
    "wave_edges_66": lambda: build(12, 30, 8, win_null=(3,), tied=True),
    "wave_edges_276": lambda: build(24, 60, 9, ts_null=(5,)),
    "family_150": lambda: build(150, 5160, 10, win_null=(17,), ts_null=(17, 90)),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    return CASES[name]()


def all_cases() -> dict:
    return {name: case(name) for name in CASES}


FULL_ROWS_LIMIT = 300  # frames of at most this many rows are kept value by value in the golden file, larger ones as digests


def frame_records(frame) -> dict:
    import dominance_cases

    return dominance_cases.frame_records(frame)


def frame_golden(frame) -> dict:
    import dominance_cases

    return dominance_cases.frame_records(frame) if len(frame) <= FULL_ROWS_LIMIT else dominance_cases.frame_digest(frame)


def inference_frame(c: dict):
    """What ``_pair_agreement`` reads of the inference: family hash, pair id, both strategies, the decision class."""
    import pandas as pd

    from farkle_ii_amd import round_robin as rr
    from farkle_ii_amd.rr_inference import DECISION_CLASSES

    pid, i, j = rr.pair_ids(c["n"])
    return pd.DataFrame({"family_hash": c["family_hash"], "pair_id": pid.astype(np.int64), "strategy_a": c["ids"][i], "strategy_b": c["ids"][j],
                         "decision_class": np.asarray(DECISION_CLASSES, dtype=object)[c["cls"]]})


def root_agreement_frame(c: dict):
    """A ``root_decision_agreement`` table with the case's counts: the columns ``_summary`` reads."""
    import pandas as pd

    pairs, available, decision, direction = (int(v) for v in c["root_summary"][:4])
    have = np.arange(pairs) < available

    def column(agree: int):
        out = np.full(pairs, None, dtype=object)
        out[have] = (np.arange(available) < agree).tolist()
        return out

    return pd.DataFrame({"agreement_available": have, "diagnostic_holm_decision_agreement": column(decision), "effect_direction_agreement": column(direction)})
