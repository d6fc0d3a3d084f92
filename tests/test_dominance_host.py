"""The host statement of the dominance graphs (``farkle_ii_amd.dominance.graph``) and the four frames built from its arrays, against
what the reference's own ``analysis/dominance.py`` produced for every case of tests/dominance_cases.py
(tests/golden/dominance_vectors.json, recorded by tools/gen_dominance_golden.py): frames equal value for value with floats by bit
pattern (a frame of more than ``FULL_ROWS_LIMIT`` rows through the SHA-256 of the same serialisation), the summary equal as JSON."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import dominance_cases as cases
from farkle_ii_amd import dominance as dom

GOLDEN = json.loads((Path(__file__).parent / "golden" / "dominance_vectors.json").read_text())


@pytest.fixture(scope="module")
def graphs():
    out = {}

    def get(name):
        if name not in out:
            c = cases.case(name)
            out[name] = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]))
        return out[name]

    return get


def test_the_golden_file_holds_every_case():
    assert sorted(GOLDEN) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_frames_and_summary_equal_the_reference(graphs, name):
    c, g, want = cases.case(name), graphs(name), GOLDEN[name]
    nodes, extremes, adjacency = g["nodes"], g["extremes"], g["adjacency"]
    frames = {"edges": dom.edges_frame(cases.inference_rows(c), c["ids"], c["delta"]),
              "fronts": dom.fronts_frame(nodes, c["strategies"], c["ids"], c["scores"]),
              "cycles": dom.cycles_frame(nodes, extremes, adjacency, c["ids"])}
    for key, frame in frames.items():
        assert cases.frame_golden(frame) == want[key], key
    got = dom.summary(nodes, c["strategies"], cases.class_counts(c), c["ids"], family_hash=want["summary"]["family_hash"])
    assert got.pop("interpretation") == dom.INTERPRETATION
    assert json.dumps(got, sort_keys=True) == json.dumps(want["summary"], sort_keys=True)


def test_shapes_the_cases_are_there_for(graphs):
    """What each designed case is meant to exercise does show in the host statement."""
    nodes = graphs("total_order_100")["nodes"]
    assert sorted(nodes["front"][:, 1]) == list(range(1, 101)) and (nodes["component_size"] == 1).all() and not nodes["cycle_length"].any()
    nodes = graphs("path_300")["nodes"]
    assert nodes["front"][:, 1].tolist() == list(range(1, 301)) and nodes["front"][:, 0].max() < 300
    nodes = graphs("ring_130")["nodes"]
    assert (nodes["cycle_length"] == 130).all() and (nodes["component_size"] == 130).all() and (nodes["front"] == 1).all()
    nodes = graphs("component_across_a_word_boundary")["nodes"]
    assert nodes["component"][62:66, 0].tolist() == [62] * 4 and nodes["component_size"][65, 1] == 4
    g = graphs("statistical_component_without_practical_edge")
    assert g["nodes"]["component_size"][0, 1] == 3 and g["extremes"]["strongest_winner"][1, 0] == dom.NONE and np.isnan(g["extremes"]["weakest_distance"][1, 0])
    g = graphs("equal_distances")  # ids 8 .. 12 sort as strings 10 11 12 8 9: the first edge in that order is 10 -> 11 = rows 2 -> 3
    assert (g["extremes"]["strongest_winner"][0, 0], g["extremes"]["strongest_loser"][0, 0]) == (2, 3)
    assert (g["extremes"]["weakest_winner"][0, 0], g["extremes"]["weakest_loser"][0, 0]) == (2, 3)
    nodes = graphs("strategy_without_any_rate")["nodes"]
    assert nodes["rate_count"][5] == 0 and np.isnan(nodes["rate_mean"][5]) and (nodes["rate_count"][:5] == 4).all()
    for name in ("dense_128", "dense_129"):
        assert graphs(name)["nodes"]["component_size"][:, 1].max() > 100
    assert (graphs("sparse_129")["nodes"]["component_size"][:, 1] > 1).sum() > 10 and graphs("sparse_129")["nodes"]["component_size"].max() < 40


def test_table_order_breaks_ties_without_a_rank():
    c = cases.case("equal_distances")
    g = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"])
    assert (g["extremes"]["strongest_winner"][0, 0], g["extremes"]["strongest_loser"][0, 0]) == (0, 1)


def test_fronts_frame_without_screening_scores():
    c = cases.case("two_3_cycles_joined")
    g = dom.graph(c["n"], c["cls"], c["low"], c["high"], c["rate"], c["delta"], rank=dom.rank_of_ids(c["ids"]))
    frame = dom.fronts_frame(g["nodes"], c["strategies"], c["ids"])
    assert frame["tournament_screening_score"].isna().all() and sorted(frame["practical_display_position_within_front"]) == [1, 1, 2, 2, 3, 3]


@pytest.mark.parametrize("bad, match", [
    (dict(n=1), "at least two"), (dict(n=8193), "at most 8192"), (dict(delta=0.0), "practical_delta must be positive"),
    (dict(cls=7), "is not one of the 7 classes"), (dict(low=np.inf), "bound is not finite"), (dict(rank=[0, 0, 1, 2]), "not a permutation")])
def test_the_host_statement_refuses_what_the_entry_refuses(bad, match):
    c = cases.case("cycle3_and_tail")
    cls, low = c["cls"].copy(), c["low"].copy()
    if "cls" in bad:
        cls[0] = bad["cls"]
    if "low" in bad:
        low[0] = bad["low"]  # pair 0 is the practical edge 0 -> 1
    with pytest.raises(ValueError, match=match):
        dom.graph(bad.get("n", c["n"]), cls, low, c["high"], c["rate"], bad.get("delta", c["delta"]), rank=bad.get("rank"))
