"""The method agreement on the CPU: the host statements and frames of ``farkle_ii_amd.structure_agreement`` against the reference's own
results (tests/golden/agreement_vectors.json, recorded by tools/gen_agreement_golden.py) on every case of tests/agreement_cases.py;
``kendall_from_counts`` and Spearman against scipy bit for bit; ``ag_pair_code`` and ``cc_row_counts`` of csrc/fk_agreement.h (built
into tests/native/agreement_host_check.hip without a GPU) against the host statements; every refusal of ``read_membership``."""
from __future__ import annotations

import itertools
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import agreement_cases as cases
from farkle_ii_amd import rr_root_diagnostics as rd
from farkle_ii_amd import structure_agreement as sa
from farkle_ii_amd.backend import CONCORDANCE_TILE

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = ROOT / "tests" / "native" / "agreement_host_check.hip"
GOLDEN = json.loads((ROOT / "tests" / "golden" / "agreement_vectors.json").read_text())


def host_results(c: dict) -> dict:
    """What the command computes for a case, every entry replaced by its host statement."""
    membership = sa.membership_from_frame(c["membership"], c["ids"])
    codes = sa.pair_codes(c["n"], c["cls"], membership["win_rate_rank"], membership["trueskill_rank"])
    counts = sa.pair_counts(codes, c["cls"])
    x, y = sa.scored_population(membership)
    concordance = sa.concordance_counts(x, y) if len(x) >= 2 else None
    return {"membership": membership, "codes": codes, "counts": counts, "concordance": concordance,
            "pairs": sa.pairs_frame(codes, c["cls"], c["ids"], membership["family_hash"]),
            "summary": sa.summary(membership, counts, concordance, rd.stability_summary(c["root_summary"]), c["execution_scope"])}


def test_the_golden_file_holds_every_case_and_is_small():
    assert sorted(GOLDEN["cases"]) == sorted(cases.CASES)
    assert (ROOT / "tests" / "golden" / "agreement_vectors.json").stat().st_size < 200_000
    assert GOLDEN["meta"]["reference_pair_agreement_seconds_family_150"] > 0.0
    assert "sha256" in GOLDEN["cases"]["family_150"]["pairs"] and "rows" in GOLDEN["cases"]["wave_edges_276"]["pairs"]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_frames_and_summary_against_the_reference(name):
    c, want = cases.case(name), GOLDEN["cases"][name]
    got = host_results(c)
    assert cases.frame_golden(got["pairs"]) == want["pairs"]
    assert got["summary"] == want["summary"]
    assert json.loads(json.dumps(got["summary"])) == want["summary"]  # (plain JSON types)
    counts = got["counts"]
    assert counts[0] == c["n"] * (c["n"] - 1) // 2 and counts[1] + counts[2] + counts[4] == counts[0]
    assert all(counts[k + 1] <= counts[k] for k in (5, 7, 9)) and counts[7] <= counts[1] and counts[9] <= counts[1]


def test_the_cases_reach_what_they_are_named_for():
    got = {name: host_results(cases.case(name)) for name in ("every_class", "null_ranks", "one_method_absent", "tied_ranks", "no_directional")}
    assert sorted(set(cases.case("every_class")["cls"].tolist())) == list(range(7))
    nulls = got["null_ranks"]["membership"]
    assert (nulls["win_rate_rank"] == 0).sum() == 2 and (nulls["trueskill_rank"] == 0).sum() == 2 and ((nulls["win_rate_rank"] == 0) & (nulls["trueskill_rank"] == 0)).sum() == 1
    absent = got["one_method_absent"]["summary"]
    assert absent["rank_agreement"] == {"spearman": None, "kendall": None} and absent["common_scored_population_count"] == 0
    assert absent["selection_conditioned_h2h"]["win_rate_trueskill_direction_agreement_fraction"] is None
    assert absent["selection_conditioned_h2h"]["h2h_trueskill_direction_agreement_fraction"] is None
    assert absent["root_specific_h2h_stability"]["available"] is False and absent["execution_scope"] == "single_root"
    assert got["tied_ranks"]["concordance"][2:].min() > 0  # ties of each kind
    assert ((got["tied_ranks"]["codes"] >> 2) & 3 == 0).any()  # equal ranks inside a pair: no preference
    assert got["no_directional"]["counts"][1] == 0 and got["no_directional"]["summary"]["selection_conditioned_h2h"]["h2h_win_rate_direction_agreement_fraction"] is None


def test_summary_without_root_diagnostics_and_its_refusals():
    c = cases.case("population_larger")
    got = host_results(c)
    bare = sa.summary(got["membership"], got["counts"], got["concordance"], None, "single_root")
    assert bare["root_specific_h2h_stability"] is None and bare["execution_scope"] == "single_root"
    assert {k: v for k, v in bare.items() if k not in ("root_specific_h2h_stability", "execution_scope")} == \
           {k: v for k, v in got["summary"].items() if k not in ("root_specific_h2h_stability", "execution_scope")}
    with pytest.raises(ValueError, match="concordance counts are required"):
        sa.summary(got["membership"], got["counts"], None, None, "single_root")
    with pytest.raises(ValueError, match="must hold 11 counts"):
        sa.summary(got["membership"], got["counts"][:10], got["concordance"], None, "single_root")


def _random_keys(rng, m: int, distinct: int) -> tuple[np.ndarray, np.ndarray]:
    return rng.integers(1, distinct + 1, size=m).astype(np.int32), rng.integers(1, distinct + 1, size=m).astype(np.int32)


@pytest.mark.filterwarnings("ignore:An input array is constant")
def test_kendall_and_spearman_equal_scipy_bit_for_bit():
    from scipy.stats import kendalltau, spearmanr

    rng = np.random.default_rng(2024)
    keys = [sa.scored_population(sa.membership_from_frame(c["membership"], c["ids"])) for c in cases.all_cases().values()]
    keys = [k for k in keys if len(k[0]) >= 2]
    for _ in range(200):
        m = int(rng.integers(2, 80))
        keys.append(_random_keys(rng, m, int(rng.choice([1, 2, 3, m, 4 * m]))))
    keys.append((1 + np.arange(50, dtype=np.int32), 1 + np.arange(50, dtype=np.int32)[::-1]))
    keys.append((np.full(9, 3, dtype=np.int32), 1 + np.arange(9, dtype=np.int32)))
    saw_none = saw_tie = 0
    for x, y in keys:
        counts = sa.concordance_counts(x, y)
        assert counts.sum() == len(x) * (len(x) - 1) // 2
        want = float(kendalltau(x.astype(np.float64), y.astype(np.float64)).statistic)
        got = sa.kendall_from_counts(counts, len(x))
        assert (got is None and np.isnan(want)) or (got is not None and np.float64(got).tobytes() == np.float64(want).tobytes()), (x, y)
        saw_none += got is None
        saw_tie += counts[2:].sum() > 0
        rho = float(spearmanr(x.astype(np.float64), y.astype(np.float64)).statistic)
        assert (sa.spearman(x, y) is None and np.isnan(rho)) or np.float64(sa.spearman(x, y)).tobytes() == np.float64(rho).tobytes()
    assert saw_none > 0 and saw_tie > 100
    assert sa.kendall_from_counts(np.zeros(5, dtype=np.int64), 1) is None and sa.spearman([1], [1]) is None


def test_concordance_counts_against_the_full_matrix():
    rng = np.random.default_rng(5)
    for m, distinct in ((2, 1), (2, 5), (17, 3), (64, 200), (301, 7)):
        x, y = _random_keys(rng, m, distinct)
        upper = np.triu(np.ones((m, m), dtype=bool), 1)
        dx, dy = np.sign(x[:, None].astype(np.int64) - x[None, :]), np.sign(y[:, None].astype(np.int64) - y[None, :])
        want = [np.count_nonzero(upper & (dx * dy > 0)), np.count_nonzero(upper & (dx * dy < 0)), np.count_nonzero(upper & (dx == 0) & (dy != 0)),
                np.count_nonzero(upper & (dx != 0) & (dy == 0)), np.count_nonzero(upper & (dx == 0) & (dy == 0))]
        assert sa.concordance_counts(x, y).tolist() == want
    with pytest.raises(ValueError, match="a key is at least 1"):
        sa.concordance_counts([1, 0], [1, 2])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not (shutil.which(HIPCC) or Path(HIPCC).exists()):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("agreement") / "agreement_host_check"
    # host side only (the checker launches no kernel), as tests/test_rr_inference_host.py builds its checker
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-o", str(exe), str(SOURCE)], check=True, capture_output=True,
                   text=True)
    return exe


def test_header_pair_code_over_every_class_and_rank_relation(checker):
    """Every class x {null, smaller, equal, larger}^2 of the two methods (and A null with B null) against ``pair_codes`` at n = 2."""
    relations = ((0, 5), (5, 0), (0, 0), (3, 9), (7, 7), (9, 3), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1))
    todo = [(cls, win, ts) for cls in range(7) for win, ts in itertools.product(relations, relations)]
    text = "".join(f"p {cls} {win[0]} {win[1]} {ts[0]} {ts[1]}\n" for cls, win, ts in todo)
    out = subprocess.run([str(checker)], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(todo) == 7 * 64
    for (cls, win, ts), got in zip(todo, out):
        assert int(got) == int(sa.pair_codes(2, [cls], win, ts)[0]), (cls, win, ts)
    assert len(set(out)) == 27  # three directions x three preferences x three preferences


def test_header_tile_counts_over_small_m(checker):
    """The kernel's tile walk on the host: one tile, a diagonal and an off-diagonal tile, a ragged last tile; with and without ties."""
    T = CONCORDANCE_TILE
    rng = np.random.default_rng(77)
    todo = [_random_keys(rng, m, distinct) for m in (2, 3, T - 1, T, T + 1, 2 * T + 1) for distinct in (1, 4, 10 * m)]
    text = "".join(f"c {len(x)} {' '.join(map(str, x))} {' '.join(map(str, y))}\n" for x, y in todo)
    out = subprocess.run([str(checker)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(todo)
    for (x, y), line in zip(todo, out):
        assert [int(v) for v in line.split()] == sa.concordance_counts(x, y).tolist(), len(x)


def test_read_membership_and_its_refusals(tmp_path):
    import pandas as pd

    c = cases.case("null_ranks")
    frame = c["membership"].copy()
    for column in ("win_rate_rank", "trueskill_rank"):  # the file's own layout: nullable integers
        frame[column] = frame[column].astype("Int64")
    path = tmp_path / "candidate_family.parquet"
    frame.to_parquet(path)
    read = sa.read_membership(path, c["ids"])
    want = sa.membership_from_frame(c["membership"], c["ids"])
    for key in ("win_rate_rank", "trueskill_rank", "population_win_rate_rank", "population_trueskill_rank"):
        assert np.array_equal(read[key], want[key]) and read[key].dtype == want[key].dtype
    assert read["win_rate_rank"].dtype == np.int32 and read["family_hash"] == cases.FAMILY_HASH
    finalist = int(np.flatnonzero(frame["final_family"])[0])

    def refused(change, match, ids=c["ids"]):
        bad = c["membership"].copy()
        change(bad)
        with pytest.raises(ValueError, match=match):
            sa.membership_from_frame(bad, ids)

    def duplicate(f):
        f.loc[1, "strategy"] = f.loc[0, "strategy"]

    refused(duplicate, "candidate provenance contains duplicate strategies")
    refused(lambda f: None, "H2H inference finalist support differs from candidate provenance", ids=c["ids"][:-1])
    refused(lambda f: f.__setitem__("final_family", True), "H2H inference finalist support differs from candidate provenance")
    refused(lambda f: f.__setitem__("family_hash", [f"h{k % 2}" for k in range(len(f))]), "candidate provenance must contain one final family hash")
    for value in (0.0, -3.0, 2.5, 2.0 ** 31, np.inf):
        refused(lambda f, v=value: f.__setitem__("win_rate_rank", f["win_rate_rank"].where(f.index != finalist, v)),
                "win_rate_rank must be a positive integer below 2\\^31 or null")
    refused(lambda f: f.__setitem__("trueskill_rank", f["trueskill_rank"].where(f.index != finalist, 0.5)), "trueskill_rank must be a positive integer")
    refused(lambda f: f.drop(columns=["configured_control"], inplace=True), "lacks the columns \\['configured_control'\\]")
    with pytest.raises(ValueError, match="duplicate strategies"):  # through the file as well
        bad = frame.copy()
        bad.loc[1, "strategy"] = bad.loc[0, "strategy"]
        bad.to_parquet(path)
        sa.read_membership(path, c["ids"])
    assert isinstance(pd.read_parquet(path)["win_rate_rank"].dtype, pd.Int64Dtype)
