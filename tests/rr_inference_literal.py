"""A literal restatement of the statistics of the reference's ``src/farkle/analysis/h2h_inference.py`` :68-295 for the tests of the
round-robin inference: scalar Python in the reference's order of floating-point operations, ``scipy.stats.norm`` for the tail and
the quantile, ``scipy.optimize.brentq`` at ``xtol = 1e-12``, ``rtol = 1e-14`` inside the reference's dyadic bracket.  Nothing here
is shared with ``farkle_ii_amd.rr_inference`` or the device header: the three are compared with each other."""
from __future__ import annotations

import math

import numpy as np
from scipy.optimize import brentq
from scipy.stats import norm

# the differences tests/native/rr_inference_host_check.hip evaluates the statistic at
DIFFERENCES = (-0.5, -0.0625, 0.0, 0.03, 0.75)
# Interval bounds of the raw difference, absolute: twice brentq's stated xtol + rtol |x| <= 1.01e-12, plus the device bracket 2^-44
BOUND_TOL = 2.5e-12


def score_test(x1: int, m1: int, x2: int, m2: int) -> tuple[float, float, float, float]:
    """:80-93 -> (difference, null_proportion, statistic, p_value)"""
    r1 = x1 / m1
    r2 = x2 / m2
    diff = r1 - r2
    pooled = (x1 + x2) / (m1 + m2)
    var = pooled * (1.0 - pooled) * (1.0 / m1 + 1.0 / m2)
    if var > 0.0:
        stat = diff / math.sqrt(var)
        return diff, pooled, stat, float(2.0 * norm.sf(abs(stat)))
    if diff == 0.0:
        return diff, pooled, 0.0, 1.0
    return diff, pooled, math.copysign(math.inf, diff), 0.0


def stat_at(x1: int, m1: int, x2: int, m2: int, delta: float) -> float:
    """:151-188"""
    seen = x1 / m1 - x2 / m2
    if delta <= -1.0:
        pa, pb = 0.0, 1.0
    elif delta >= 1.0:
        pa, pb = 1.0, 0.0
    elif delta == 0.0:
        pa = pb = (x1 + x2) / (m1 + m2)
    else:
        mm = m1 + m2
        xx = x1 + x2
        a2 = (m1 + 2 * m2) * delta - mm - xx
        a1 = (x2 * delta - mm - 2 * x2) * delta + xx
        a0 = x2 * delta * (1.0 - delta)
        qq = (a2 / (3 * mm)) ** 3 - a1 * a2 / (6 * mm**2) + a0 / (2 * mm)
        rad = (a2 / (3 * mm)) ** 2 - a1 / (3 * mm)
        pp = math.copysign(math.sqrt(max(0.0, rad)), qq) if qq != 0.0 else 0.0
        if pp == 0.0:
            pb = -a2 / (3 * mm)
        else:
            clipped = max(-1.0, min(1.0, qq / pp**3))
            theta = (math.pi + math.acos(clipped)) / 3.0
            pb = 2.0 * pp * math.cos(theta) - a2 / (3 * mm)
        pa = pb + delta
        pa = max(0.0, min(1.0, pa))
        pb = max(0.0, min(1.0, pb))
    var = pa * (1.0 - pa) / m1 + pb * (1.0 - pb) / m2
    top = seen - delta
    if var > 0.0:
        return top / math.sqrt(var)
    if top == 0.0:
        return 0.0
    return math.copysign(math.inf, top)


def bound(x1: int, m1: int, x2: int, m2: int, seen: float, edge: float, crit: float) -> float:
    """:203-231"""
    if seen == edge:
        return edge

    def g(delta: float) -> float:
        s = stat_at(x1, m1, x2, m2, delta)
        assert not math.isnan(s)
        if math.isinf(s):
            return 1.0
        return abs(s) - crit

    last = seen
    reach = edge - seen
    for e in range(52, -1, -1):
        trial = seen + reach * 2.0**-e
        if trial == last:
            continue
        if g(trial) >= 0.0:
            return float(brentq(g, min(last, trial), max(last, trial), xtol=1e-12, rtol=1e-14))
        last = trial
    raise AssertionError("no bracket")


def interval(x1: int, m1: int, x2: int, m2: int, alpha: float) -> tuple[float, float]:
    """:244-277"""
    seen = x1 / m1 - x2 / m2
    if seen > 0.0:
        lo, hi = interval(x2, m2, x1, m1, alpha)
        return -hi, -lo
    crit = float(norm.isf(alpha / 2.0))
    lo = bound(x1, m1, x2, m2, seen, -1.0, crit)
    hi = bound(x1, m1, x2, m2, seen, 1.0, crit)
    if x1 == x2 and m1 == m2:
        widest = max(abs(lo), abs(hi))
        return -widest, widest
    return lo, hi


def holm(p: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """:283-295"""
    m = len(p)
    order = np.argsort(p, kind="mergesort")
    stepped = np.maximum.accumulate(np.asarray([(m - k) * p[at] for k, at in enumerate(order)], dtype=float))
    adjusted = np.empty(m, dtype=float)
    adjusted[order] = np.minimum(1.0, stepped)
    place = np.empty(m, dtype=np.int64)
    place[order] = np.arange(1, m + 1, dtype=np.int64)
    return adjusted, place
