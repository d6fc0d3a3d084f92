"""Dominance fronts and cycle groups of a round robin: the reference's ``src/farkle/analysis/dominance.py`` over the decision classes
of ``rr_inference``.

``Engine.dominance_graph`` (``fk_dominance_graph``) and ``Engine.rr_dominance`` (``fk_rr_dominance``) build both of the reference's
directed graphs — index 0 practical, index 1 statistical — as dense bit matrices on the device and return, per table row, the strongly
connected component, its size, the front of the condensation, the shortest cycle length, wins, losses and the round-robin mean win
rate, and per component the strongest and weakest internal practical edge.  This module is the host side:

* ``graph`` — the host statement of the entry: NumPy over the same bit matrices (``[n, ceil(n / 64)]`` uint64 words), iterative, no
  recursion; it returns what ``Engine.dominance_graph`` returns and the tests compare the two bit for bit;
* ``rank_of_ids`` — the order that breaks ties between equally strong edges: the reference orders strategies as strings;
* ``edges_frame`` / ``fronts_frame`` / ``cycles_frame`` / ``summary`` — the reference's four digest artifacts (``_edge_frames``
  :275-347, ``_descriptive_scores`` + ``_front_frame`` :350-446, ``_cycle_frame`` :489-577, the summary :662-698) in its columns,
  dtypes and row order, from those arrays.  Strategies are named by ``str(id)``, as the reference names them.

``tournament_screening_score`` is a caller-supplied mapping ``{strategy id: score}``: it is the third key of the display order inside
a front and nothing else.  Without it the column is null and that sort key is constant.  The across-k performance artifact the
reference reads it from is not produced by this package.  Also left out: ``family_hash`` unless the caller gives one, sidecars and
the stage stamp.
"""
from __future__ import annotations

import json
from typing import Any, Mapping

import numpy as np

from .backend import DOM_EXTREME_DTYPE, DOM_MAX_N, DOM_NODE_DTYPE, RR_CLASSES
from .round_robin import pair_count, pair_ids
from .rr_inference import DECISION_CLASSES

GRAPHS = ("practical", "statistical")
NONE = 0xFFFFFFFF  # a component without an internal practical edge
EDGE_COLUMNS = ("graph_type", "pair_id", "winner", "loser", "decision_class", "d_ab", "simultaneous_d_low", "simultaneous_d_high",
                "practical_delta", "practical_distance_beyond_threshold")
CYCLE_COLUMNS = ("graph_type", "cycle_group", "cycle_size", "members_json", "strategy", "front", "internal_practical_edge_evidence_available",
                 "strongest_internal_practical_winner", "strongest_internal_practical_loser", "strongest_internal_practical_distance",
                 "weakest_internal_practical_winner", "weakest_internal_practical_loser", "weakest_internal_practical_distance",
                 "representative_shortest_cycle_json")
INTERPRETATION = ("Fronts are partial dominance layers; cycle members and unresolved pairs remain explicit and display order does not add "
                  "inferential edges.")


def words(n: int) -> int:
    """64-bit words of one matrix row."""
    return (int(n) + 63) // 64


def pack_bits(matrix: np.ndarray) -> np.ndarray:
    """bool ``[rows, n]`` -> uint64 ``[rows, words(n)]``, bit ``j & 63`` of word ``j >> 6``."""
    rows, n = matrix.shape
    padded = np.zeros((rows, words(n) * 64), dtype=bool)
    padded[:, :n] = matrix
    return np.packbits(padded, axis=1, bitorder="little").view("<u8")


def unpack_bits(packed: np.ndarray, n: int) -> np.ndarray:
    """uint64 ``[rows, words(n)]`` -> bool ``[rows, n]``."""
    packed = np.ascontiguousarray(packed, dtype="<u8")
    return np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def rank_of_ids(strategy_ids) -> np.ndarray:
    """``rank[row]``: the position of ``str(strategy_ids[row])`` among the ids sorted as strings."""
    names = [str(int(v)) for v in strategy_ids]
    rank = np.empty(len(names), dtype=np.uint32)
    rank[sorted(range(len(names)), key=names.__getitem__)] = np.arange(len(names), dtype=np.uint32)
    return rank


def check_inputs(n: int, decision_class, sim_d_low, sim_d_high, practical_delta: float, rank) -> None:
    """What ``fk_dominance_graph`` refuses, with the same conditions."""
    if n < 2:
        raise ValueError(f"a dominance graph needs at least two strategies, got {n}")
    if n > DOM_MAX_N:
        raise ValueError(f"a dominance graph holds at most {DOM_MAX_N} strategies, got {n}")
    if not practical_delta > 0.0:
        raise ValueError(f"practical_delta must be positive, got {practical_delta}")
    if len(decision_class) and int(decision_class.max()) >= RR_CLASSES:
        raise ValueError(f"decision class {int(decision_class.max())} is not one of the {RR_CLASSES} classes")
    needed = np.where(decision_class == 0, sim_d_low, np.where(decision_class == 1, sim_d_high, 0.0))
    if not np.isfinite(needed).all():
        raise ValueError(f"pair {int(np.flatnonzero(~np.isfinite(needed))[0])} is a practical dominance whose simultaneous bound is not finite")
    if rank is not None and not np.array_equal(np.sort(rank), np.arange(n)):
        raise ValueError(f"rank is not a permutation of 0 .. {n - 1}")


def distances(decision_class, sim_d_low, sim_d_high, practical_delta: float) -> np.ndarray:
    """``practical_distance_beyond_threshold`` (:315-319) of every pair, NaN where the pair is no practical edge."""
    return np.where(decision_class == 0, sim_d_low - practical_delta, np.where(decision_class == 1, -sim_d_high - practical_delta, np.nan))


def _closure(adj: np.ndarray, n: int) -> np.ndarray:
    """Warshall on packed rows: ``reach[i]`` gets bit ``j`` when a path of one edge or more leads from ``i`` to ``j``."""
    reach = adj.copy()
    for k in range(n):
        rows = np.flatnonzero((reach[:, k >> 6] >> np.uint64(k & 63)) & np.uint64(1))
        if len(rows):
            reach[rows] |= reach[k]
    return reach


def _fronts(edges: np.ndarray, comp: np.ndarray, n: int) -> np.ndarray:
    """Kahn's rounds on the condensation: a round takes every node whose component no untaken other component has an edge into."""
    source, target = np.nonzero(edges & (comp[:, None] != comp[None, :]))  # sorted by source
    begin = np.searchsorted(source, np.arange(n + 1))
    degree = np.bincount(comp[target], minlength=n)
    front = np.zeros(n, dtype=np.uint32)
    level = 0
    while (front == 0).any():
        level += 1
        layer = np.flatnonzero((front == 0) & (degree[comp] == 0))
        if not len(layer):
            raise RuntimeError("condensation graph unexpectedly contains a cycle")
        front[layer] = level
        counts = begin[layer + 1] - begin[layer]
        if counts.sum():
            at = np.repeat(begin[layer] - np.concatenate(([0], np.cumsum(counts)[:-1])), counts) + np.arange(counts.sum())
            np.subtract.at(degree, comp[target[at]], 1)
    return front


def _cycle_lengths(edges: np.ndarray, comp: np.ndarray, size: np.ndarray) -> np.ndarray:
    """Per node of a component of two or more: breadth-first search on frontiers inside the component until one holds a node with an
    edge back to the start."""
    out = np.zeros(len(comp), dtype=np.uint32)
    for head in np.flatnonzero((comp == np.arange(len(comp))) & (size > 1)):
        members = np.flatnonzero(comp == head)
        sub = edges[np.ix_(members, members)]
        for s in range(len(members)):
            frontier = sub[s].copy()
            seen = frontier.copy()
            level = 1
            while not (frontier & sub[:, s]).any():
                frontier = sub[frontier].any(axis=0) & ~seen
                frontier[s] = False
                if not frontier.any():
                    raise RuntimeError("a strongly connected component lacks a cycle through one of its nodes")
                seen |= frontier
                level += 1
            out[members[s]] = level + 1
    return out


def graph(n: int, decision_class, sim_d_low, sim_d_high, balanced_rate, practical_delta: float = 0.03, rank=None) -> dict:
    """The host statement of ``fk_dominance_graph``: ``{"nodes": DOM_NODE_DTYPE [n], "extremes": DOM_EXTREME_DTYPE [2, n], "adjacency":
    uint64 [2, n, words(n)]}`` from the pairs' classes, simultaneous bounds and rates in pair-id order."""
    n = int(n)
    cls = np.asarray(decision_class, dtype=np.uint8).reshape(-1)
    low, high, rate = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (sim_d_low, sim_d_high, balanced_rate))
    rank = None if rank is None else np.asarray(rank, dtype=np.int64)
    check_inputs(n, cls, low, high, float(practical_delta), rank)
    if not len(cls) == len(low) == len(high) == len(rate) == pair_count(n):
        raise ValueError(f"a table of {n} strategies has {pair_count(n)} pairs")
    order = np.arange(n, dtype=np.int64) if rank is None else rank
    _, i, j = pair_ids(n)
    winner, loser = np.where(cls & 1, j, i), np.where(cls & 1, i, j)
    nodes = np.zeros(n, dtype=DOM_NODE_DTYPE)
    extremes = np.zeros((2, n), dtype=DOM_EXTREME_DTYPE)
    for name in ("strongest_winner", "strongest_loser", "weakest_winner", "weakest_loser"):
        extremes[name] = NONE
    extremes["strongest_distance"] = extremes["weakest_distance"] = np.nan
    adjacency = np.zeros((2, n, words(n)), dtype=np.uint64)
    distance = distances(cls, low, high, float(practical_delta))
    for g, limit in enumerate((2, 4)):
        edges = np.zeros((n, n), dtype=bool)
        edges[winner[cls < limit], loser[cls < limit]] = True
        adjacency[g] = pack_bits(edges)
        reach = unpack_bits(_closure(adjacency[g], n), n)
        same = reach & reach.T
        np.fill_diagonal(same, True)
        comp = same.argmax(axis=1)
        size = same.sum(axis=1)
        nodes["component"][:, g], nodes["component_size"][:, g] = comp, size
        nodes["wins"][:, g], nodes["losses"][:, g] = edges.sum(axis=1), edges.sum(axis=0)
        nodes["front"][:, g] = _fronts(edges, comp, n)
        nodes["cycle_length"][:, g] = _cycle_lengths(edges, comp, size)
        inside = np.flatnonzero((cls < 2) & (comp[i] == comp[j]))  # the practical edges with both ends in one component of THIS graph
        for sign, prefix in ((-1.0, "strongest"), (1.0, "weakest")):
            by = np.lexsort((order[loser[inside]], order[winner[inside]], sign * distance[inside], comp[i[inside]]))
            picked = inside[by]
            first = picked[np.concatenate(([True], comp[i[picked]][1:] != comp[i[picked]][:-1]))] if len(picked) else picked
            at = comp[i[first]]
            extremes[f"{prefix}_winner"][g, at], extremes[f"{prefix}_loser"][g, at] = winner[first], loser[first]
            extremes[f"{prefix}_distance"][g, at] = distance[first]
    # the mean rate: per strategy its opponents in table order ARE its pairs in pair-id order; one vector step per opponent keeps every
    # strategy's sum left to right
    share = np.full((n, n), np.nan)
    share[i, j], share[j, i] = rate, 1.0 - rate
    total, count = np.zeros(n), np.zeros(n, dtype=np.uint64)
    for opponent in range(n):
        have = ~np.isnan(share[:, opponent])
        total[have] = total[have] + share[have, opponent]
        count[have] += np.uint64(1)
    nodes["rate_count"] = count
    with np.errstate(divide="ignore", invalid="ignore"):
        nodes["rate_mean"] = np.where(count > 0, total / count.astype(np.float64), np.nan)
    return {"nodes": nodes, "extremes": extremes, "adjacency": adjacency}


# ---- the frames ----
def _names(strategy_ids, n: int) -> list[str]:
    ids = np.arange(n, dtype=np.int64) if strategy_ids is None else np.asarray(strategy_ids, dtype=np.int64).reshape(-1)
    if len(ids) != n:
        raise ValueError(f"strategy_ids must name the {n} rows of the table")
    return [str(int(v)) for v in ids]


def edges_frame(rows: np.ndarray, strategy_ids=None, practical_delta: float = 0.03):
    """``_edge_frames``' table from the pair rows of ``Engine.rr_inference`` / ``rr_inference.infer`` (every pair of the table): per
    directed pair its statistical row, then — for a practical dominance — its practical row."""
    import pandas as pd

    cls = rows["decision_class"].astype(np.int64)
    n = int(rows["strategy_b"].max()) + 1 if len(rows) else 0
    names = np.asarray(_names(strategy_ids, n if strategy_ids is None else len(strategy_ids)), dtype=object)
    directed = np.flatnonzero(cls < 4)
    if not len(directed):
        return pd.DataFrame([], columns=list(EDGE_COLUMNS))
    copies = np.where(cls[directed] < 2, 2, 1)
    at = np.repeat(directed, copies)
    practical = np.concatenate(([False], at[1:] == at[:-1]))  # the second copy of a pair
    a, b = names[rows["strategy_a"][at]], names[rows["strategy_b"][at]]
    odd = (cls[at] & 1) == 1
    distance = distances(cls[at], rows["simultaneous_d_low"][at], rows["simultaneous_d_high"][at], float(practical_delta))
    return pd.DataFrame({
        "graph_type": np.where(practical, "practical", "statistical").astype(object),
        "pair_id": rows["pair_id"][at].astype(np.int64),
        "winner": np.where(odd, b, a), "loser": np.where(odd, a, b),
        "decision_class": np.asarray(DECISION_CLASSES, dtype=object)[cls[at]],
        "d_ab": rows["d_ab"][at].astype(np.float64),
        "simultaneous_d_low": rows["simultaneous_d_low"][at].astype(np.float64),
        "simultaneous_d_high": rows["simultaneous_d_high"][at].astype(np.float64),
        "practical_delta": np.full(len(at), float(practical_delta)),
        "practical_distance_beyond_threshold": np.where(practical, distance, np.nan),
    })[list(EDGE_COLUMNS)]


def _components(nodes: np.ndarray, names: list[str], g: int) -> tuple[list[tuple[str, ...]], dict[int, str]]:
    """The components of graph ``g`` of two or more, as sorted tuples of names in sorted order, and ``{smallest row: cycle id}``."""
    heads = np.flatnonzero((nodes["component"][:, g] == np.arange(len(nodes))) & (nodes["component_size"][:, g] > 1))
    members = {int(h): tuple(sorted(names[r] for r in np.flatnonzero(nodes["component"][:, g] == h))) for h in heads}
    ordered = sorted(members.items(), key=lambda item: item[1])
    return [m for _, m in ordered], {h: f"{GRAPHS[g]}_cycle_{index:03d}" for index, (h, _) in enumerate(ordered, 1)}


def fronts_frame(nodes: np.ndarray, strategies: np.ndarray, strategy_ids=None, screening_scores: Mapping[int, float] | None = None):
    """``_descriptive_scores`` + ``_front_frame``: one row per strategy, in the final order (practical front, display position).
    ``strategies`` is the per-strategy table of the inference (``rr_inference.STRATEGY_CLASS_COLS``): completion rate and viability."""
    import pandas as pd

    n = len(nodes)
    names = _names(strategy_ids, n)
    ids = [int(v) for v in names]
    st = np.asarray(strategies, dtype=np.int64)
    cycle_ids = [_components(nodes, names, g)[1] for g in range(2)]
    rows: list[dict[str, Any]] = []
    for r in sorted(range(n), key=names.__getitem__):
        operational, inferential = bool(st[r, 10]), bool(st[r, 11])
        score = None if screening_scores is None else float(screening_scores[ids[r]])
        rows.append({
            "strategy": names[r],
            "round_robin_mean_win_rate": float(nodes["rate_mean"][r]) if nodes["rate_count"][r] else None,
            "completed_pair_estimate_count": int(nodes["rate_count"][r]),
            "planned_opponent_count": n - 1,
            "candidate_completion_rate": float(st[r, 8]) / float(st[r, 7]) if st[r, 7] else float("nan"),
            "operationally_viable": operational,
            "inferentially_viable": inferential,
            "candidate_claim_eligible": operational and inferential,
            "practical_wins": int(nodes["wins"][r, 0]),
            "practical_losses": int(nodes["losses"][r, 0]),
            "practical_net_wins": int(nodes["wins"][r, 0]) - int(nodes["losses"][r, 0]),
            "statistical_wins": int(nodes["wins"][r, 1]),
            "statistical_losses": int(nodes["losses"][r, 1]),
            "tournament_screening_score": score,
            "practical_front": int(nodes["front"][r, 0]),
            "statistical_front": int(nodes["front"][r, 1]),
            "practical_cycle_group": cycle_ids[0].get(int(nodes["component"][r, 0])),
            "statistical_cycle_group": cycle_ids[1].get(int(nodes["component"][r, 1])),
        })
    output = pd.DataFrame(rows)
    keys = ["round_robin_mean_win_rate", "practical_net_wins", "tournament_screening_score", "strategy"]
    for graph_type in GRAPHS:  # the position inside a front: one stable sort by (front, keys), then a count per front
        front = f"{graph_type}_front"
        ordered = output.sort_values([front, *keys], ascending=[True, False, False, False, True], kind="mergesort")
        output[f"{graph_type}_display_position_within_front"] = (ordered.groupby(front).cumcount() + 1).reindex(output.index).astype(int)
    output["display_order_is_inferential"] = False
    return output.sort_values(["practical_front", "practical_display_position_within_front"], kind="mergesort").reset_index(drop=True)


def representative_cycle(members: list[int], adjacency_rows: np.ndarray, starts: list[int], names: list[str]) -> tuple[str, ...]:
    """The reference's representative shortest cycle of one component (:455-486): its breadth-first search, neighbours in name order,
    from ``starts`` — the members whose shortest cycle is the component's shortest; every other start yields a longer candidate, which
    the minimum by (length, canonical rotation) drops.  ``adjacency_rows``: bool ``[n, n]``."""
    inside = sorted(members, key=names.__getitem__)
    neighbours = {m: [v for v in inside if adjacency_rows[m, v]] for m in inside}
    candidates: list[tuple[str, ...]] = []
    for start in starts:
        queue = [(v, (start, v)) for v in neighbours[start]]
        visited = set(neighbours[start])
        cursor = 0
        while cursor < len(queue):
            node, path = queue[cursor]
            cursor += 1
            closed = False
            for v in neighbours[node]:
                if v == start:
                    closed = True
                    break
                if v not in visited:
                    visited.add(v)
                    queue.append((v, path + (v,)))
            if closed:
                cycle = tuple(names[v] for v in path)
                candidates.append(min(cycle[k:] + cycle[:k] for k in range(len(cycle))))
                break
    if not candidates:
        raise RuntimeError(f"strongly connected component lacks a directed cycle: {members}")
    return min(candidates, key=lambda cycle: (len(cycle), cycle))


def cycles_frame(nodes: np.ndarray, extremes: np.ndarray, adjacency: np.ndarray, strategy_ids=None):
    """``_cycle_frame``: one row per member of every component of two or more, practical graph first."""
    import pandas as pd

    n = len(nodes)
    names = _names(strategy_ids, n)
    row_of = {name: r for r, name in enumerate(names)}
    rows: list[dict[str, Any]] = []
    for g, graph_type in enumerate(GRAPHS):
        components, cycle_ids = _components(nodes, names, g)
        edges = unpack_bits(adjacency[g], n)
        for members in components:
            member_rows = [row_of[m] for m in members]
            head = int(nodes["component"][member_rows[0], g])
            lengths = nodes["cycle_length"][member_rows, g]
            starts = [r for r, length in zip(member_rows, lengths) if length == lengths.min()]
            cycle = representative_cycle(member_rows, edges, sorted(starts, key=names.__getitem__), names)
            e = extremes[g, head]
            have = int(e["strongest_winner"]) != NONE
            for member in members:
                rows.append({
                    "graph_type": graph_type,
                    "cycle_group": cycle_ids[head],
                    "cycle_size": len(members),
                    "members_json": json.dumps(list(members), separators=(",", ":")),
                    "strategy": member,
                    "front": int(nodes["front"][row_of[member], g]),
                    "internal_practical_edge_evidence_available": have,
                    "strongest_internal_practical_winner": names[int(e["strongest_winner"])] if have else None,
                    "strongest_internal_practical_loser": names[int(e["strongest_loser"])] if have else None,
                    "strongest_internal_practical_distance": float(e["strongest_distance"]) if have else None,
                    "weakest_internal_practical_winner": names[int(e["weakest_winner"])] if have else None,
                    "weakest_internal_practical_loser": names[int(e["weakest_loser"])] if have else None,
                    "weakest_internal_practical_distance": float(e["weakest_distance"]) if have else None,
                    "representative_shortest_cycle_json": json.dumps(list(cycle), separators=(",", ":")),
                })
    return pd.DataFrame(rows, columns=list(CYCLE_COLUMNS))


def summary(nodes: np.ndarray, strategies: np.ndarray, class_counts, strategy_ids=None, family_hash: str | None = None) -> dict:
    """The reference's ``dominance_summary.json`` (:662-698)."""
    n = len(nodes)
    names = _names(strategy_ids, n)
    st = np.asarray(strategies, dtype=np.int64)
    eligible = (st[:, 10] != 0) & (st[:, 11] != 0)
    winners = sorted(names[r] for r in np.flatnonzero(eligible & (nodes["wins"][:, 0] == n - 1)))
    if len(winners) > 1:
        raise RuntimeError("more than one strategy directly dominates every finalist")
    return {
        "family_hash": family_hash,
        "finalist_count": n,
        "unordered_pair_count": pair_count(n),
        "decision_counts": {name: int(v) for name, v in zip(DECISION_CLASSES, class_counts) if int(v)},
        "practical_edge_count": int(nodes["wins"][:, 0].sum()),
        "statistical_edge_count": int(nodes["wins"][:, 1].sum()),
        "practical_cycle_group_count": len(_components(nodes, names, 0)[0]),
        "statistical_cycle_group_count": len(_components(nodes, names, 1)[0]),
        "practical_front_count": int(nodes["front"][:, 0].max()),
        "statistical_front_count": int(nodes["front"][:, 1].max()),
        "unique_best": winners[0] if winners else None,
        "unique_best_claim_permitted": bool(winners),
        "unique_best_rule": "direct_practical_dominance_over_every_other_finalist",
        "operationally_nonviable_candidates": sorted(names[r] for r in np.flatnonzero(st[:, 10] == 0)),
        "inferentially_nonviable_candidates": sorted(names[r] for r in np.flatnonzero(st[:, 11] == 0)),
        "display_order_is_inferential": False,
        "interpretation": INTERPRETATION,
    }
