"""The dominance graphs of a round robin in plain Python on adjacency lists: what the reference's ``analysis/dominance.py`` computes from
the decided pairs, stated anew for the tests of large tables (tests/test_dominance_size_host.py, _gpu.py).  It shares no code with
``farkle_ii_amd/dominance.py`` — that host statement works on dense n x n matrices and takes 35 s at 8 192 strategies; this one walks
edge lists and takes well under a second there.

``graph(n, edges, low, high, rate, delta, rank)`` starts from the case's edge list ``(winner, loser, practical)``, not from the decision
classes, and returns the entry's ``nodes`` / ``extremes`` / ``adjacency`` arrays.  Index 0 is the practical graph (the practical edges),
index 1 the statistical one (every edge).  The steps are separate functions, so that a case with closed-form components and cycle lengths
(a ring over thousands of rows, where a search per member would cost n^2 steps) can take only the rest from here."""
from __future__ import annotations

import numpy as np

from farkle_ii_amd.backend import DOM_EXTREME_DTYPE, DOM_NODE_DTYPE

NONE = 0xFFFFFFFF


def adjacency_lists(n: int, winner, loser) -> tuple[list, list]:
    """``(succ, pred)``: per row the rows it beats and the rows that beat it."""
    succ, pred = [[] for _ in range(n)], [[] for _ in range(n)]
    for w, l in zip(np.asarray(winner).tolist(), np.asarray(loser).tolist()):
        succ[w].append(l)
        pred[l].append(w)
    return succ, pred


def packed(n: int, winner, loser) -> np.ndarray:
    """uint64 ``[n, ceil(n / 64)]``: bit ``l & 63`` of word ``l >> 6`` of row ``w`` for every edge."""
    words = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
    winner, loser = np.asarray(winner, dtype=np.int64), np.asarray(loser, dtype=np.int64)
    np.bitwise_or.at(words, (winner, loser >> 6), np.uint64(1) << (loser & 63).astype(np.uint64))
    return words


def components(n: int, succ: list) -> list:
    """Tarjan, iterative: per row the smallest row of its strongly connected component."""
    index, lowest, on_stack, comp = [-1] * n, [0] * n, [False] * n, [-1] * n
    stack, counter = [], 0
    for root in range(n):
        if index[root] != -1:
            continue
        index[root] = lowest[root] = counter
        counter += 1
        stack.append(root)
        on_stack[root] = True
        work = [(root, 0)]
        while work:
            v, k = work[-1]
            if k < len(succ[v]):
                work[-1] = (v, k + 1)
                u = succ[v][k]
                if index[u] == -1:
                    index[u] = lowest[u] = counter
                    counter += 1
                    stack.append(u)
                    on_stack[u] = True
                    work.append((u, 0))
                elif on_stack[u] and index[u] < lowest[v]:
                    lowest[v] = index[u]
                continue
            work.pop()
            if work and lowest[v] < lowest[work[-1][0]]:
                lowest[work[-1][0]] = lowest[v]
            if lowest[v] == index[v]:
                members = []
                while True:
                    u = stack.pop()
                    on_stack[u] = False
                    members.append(u)
                    if u == v:
                        break
                head = min(members)
                for u in members:
                    comp[u] = head
    return comp


def fronts(n: int, succ: list, comp: list) -> list:
    """Layer peeling of the condensation: layer 1 holds the components no other component has an edge into, layer k + 1 those that have
    none once the layers up to k are gone.  A row has its component's layer."""
    members: dict[int, list] = {}
    for v in range(n):
        members.setdefault(comp[v], []).append(v)
    entering = dict.fromkeys(members, 0)
    for v in range(n):
        for u in succ[v]:
            if comp[u] != comp[v]:
                entering[comp[u]] += 1
    front = [0] * n
    layer, level = [h for h, d in entering.items() if d == 0], 0
    while layer:
        level += 1
        following = []
        for head in layer:
            for v in members[head]:
                front[v] = level
                for u in succ[v]:
                    if comp[u] != head:
                        entering[comp[u]] -= 1
                        if entering[comp[u]] == 0:
                            following.append(comp[u])
        layer = following
    if 0 in front:
        raise RuntimeError("the condensation has a cycle")
    return front


def cycle_length(start: int, succ: list, pred: list, comp: list) -> int:
    """The shortest cycle through ``start``, 0 for a component of one: breadth-first inside the component; rows are found in order of
    their distance, so the first one found that beats ``start`` closes the shortest cycle."""
    c = comp[start]
    closing = {v for v in pred[start] if comp[v] == c}
    if not closing:
        return 0
    distance = {start: 0}
    queue = [start]
    for v in queue:
        for u in succ[v]:
            if comp[u] != c or u in distance:
                continue
            distance[u] = distance[v] + 1
            if u in closing:
                return distance[u] + 1
            queue.append(u)
    raise RuntimeError("a strongly connected component lacks a cycle through one of its rows")


def structure(n: int, winner, loser) -> dict:
    """component, component_size, front, cycle_length, wins, losses of one graph, each a list or array over the rows."""
    succ, pred = adjacency_lists(n, winner, loser)
    comp = components(n, succ)
    size = np.bincount(comp, minlength=n)[comp]
    return {"component": comp, "component_size": size, "front": fronts(n, succ, comp),
            "cycle_length": [cycle_length(v, succ, pred, comp) if size[v] > 1 else 0 for v in range(n)],
            "wins": np.bincount(winner, minlength=n), "losses": np.bincount(loser, minlength=n)}


def rates(n: int, rate) -> tuple[np.ndarray, np.ndarray]:
    """``(rate_count, rate_mean)``: per strategy the share it won of every pair that has a rate, summed over its opponents in table order —
    which is its pairs in pair-id order — left to right.  One step per opponent, each a vector over the strategies."""
    rate = np.asarray(rate, dtype=np.float64)
    rows = np.arange(n, dtype=np.int64)
    begin = rows * (2 * n - rows - 1) // 2  # the pair id of (row, row + 1)
    total, count = np.zeros(n), np.zeros(n, dtype=np.uint64)
    share = np.empty(n)
    for opponent in range(n):
        share[opponent] = np.nan
        share[opponent + 1:] = 1.0 - rate[begin[opponent]:begin[opponent] + n - opponent - 1]  # the pair (opponent, s): s is its B
        share[:opponent] = rate[begin[:opponent] + (opponent - 1 - rows[:opponent])]            # the pair (s, opponent): s is its A
        have = ~np.isnan(share)
        np.add(total, share, out=total, where=have)
        count += have.astype(np.uint64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return count, np.where(count > 0, total / count.astype(np.float64), np.nan)


def extremes(n: int, winner, loser, practical, comp, low, high, delta: float, rank=None) -> np.ndarray:
    """``DOM_EXTREME_DTYPE [n]`` of one graph with components ``comp``: at a component's smallest row its strongest and its weakest
    practical edge with both ends inside — by the distance beyond the threshold (one subtraction), ties to the smallest
    ``(rank[winner], rank[loser])``; "none" at every other row and for a component without such an edge."""
    out = np.zeros(n, dtype=DOM_EXTREME_DTYPE)
    for name in ("strongest_winner", "strongest_loser", "weakest_winner", "weakest_loser"):
        out[name] = NONE
    out["strongest_distance"] = out["weakest_distance"] = np.nan
    comp = np.asarray(comp)
    winner, loser = np.asarray(winner, dtype=np.int64), np.asarray(loser, dtype=np.int64)
    inside = np.flatnonzero(np.asarray(practical, dtype=bool) & (comp[winner] == comp[loser]))
    w, l = winner[inside], loser[inside]
    a, b = np.minimum(w, l), np.maximum(w, l)
    pair = a * (2 * n - a - 1) // 2 + b - a - 1
    delta = np.float64(delta)
    distance = np.where(w == a, np.asarray(low, dtype=np.float64)[pair] - delta, -np.asarray(high, dtype=np.float64)[pair] - delta)
    order = list(range(n)) if rank is None else [int(r) for r in rank]
    found: dict[int, list] = {}
    for d, u, v in zip(distance.tolist(), w.tolist(), l.tolist()):
        found.setdefault(int(comp[u]), []).append((d, order[u], order[v], u, v))
    for head, items in found.items():
        weakest = min(items)
        strongest = min((-d, ru, rv, u, v) for d, ru, rv, u, v in items)
        out[head] = (strongest[3], strongest[4], weakest[3], weakest[4], -strongest[0], weakest[0])
    return out


def graph(n: int, edges, low, high, rate, delta: float, rank=None, structures=None) -> dict:
    """``{"nodes": DOM_NODE_DTYPE [n], "extremes": DOM_EXTREME_DTYPE [2, n], "adjacency": uint64 [2, n, words]}``.  ``structures``: the
    two graphs' ``structure`` dictionaries where the caller knows them in closed form."""
    winner, loser, practical = (np.asarray(a) for a in edges)
    practical = practical.astype(bool)
    nodes = np.zeros(n, dtype=DOM_NODE_DTYPE)
    both = np.zeros((2, n), dtype=DOM_EXTREME_DTYPE)
    adjacency = np.zeros((2, n, (n + 63) // 64), dtype=np.uint64)
    for g, chosen in enumerate((practical, np.ones(len(winner), dtype=bool))):
        w, l = winner[chosen], loser[chosen]
        s = structure(n, w, l) if structures is None else structures[g]
        for name in ("component", "component_size", "front", "cycle_length", "wins", "losses"):
            nodes[name][:, g] = s[name]
        both[g] = extremes(n, winner, loser, practical, s["component"], low, high, delta, rank)
        adjacency[g] = packed(n, w, l)
    nodes["rate_count"], nodes["rate_mean"] = rates(n, rate)
    return {"nodes": nodes, "extremes": both, "adjacency": adjacency}


def of_case(c: dict, rank="ids", structures=None) -> dict:
    """``graph`` of a case of tests/dominance_size_cases.py; ``rank``: "ids" for the string order of the case's ids, None for table order."""
    if isinstance(rank, str):
        names = [str(int(v)) for v in c["ids"]]
        rank = np.empty(len(names), dtype=np.int64)
        rank[sorted(range(len(names)), key=names.__getitem__)] = np.arange(len(names))
    return graph(c["n"], c["edges"], c["low"], c["high"], c["rate"], c["delta"], rank, structures)
