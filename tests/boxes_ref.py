"""A numpy / pure-Python restatement of the dominated-space box decomposition, written from the specification in
``include/dkg.h`` ("Dominated-space boxes"), not from the kernels: explicit staircases kept as sorted lists, strips
taken in ascending order.  Shared by ``test_boxes_host.py`` and ``test_gpu_boxes.py``, with the input cases.

``boxes(Y, ref) -> (lo [n, m], hi [n, m])``; every corner is the Python float of an input value or of ``ref``.
"""

from __future__ import annotations

import bisect
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52


def qualifying(Y, ref):
    Y = np.asarray(Y, dtype=np.float64)
    return [i for i in range(Y.shape[0]) if all(Y[i, c] > ref[c] for c in range(Y.shape[1]))]


def _boxes1(Y, ref, idx):
    best = max(float(Y[i, 0]) for i in idx)
    # the maximum as the first point that attains it
    return [((float(ref[0]),), (best,))]


def _boxes2(Y, ref, idx):
    pts = []
    for i in idx:
        a, b = float(Y[i, 0]), float(Y[i, 1])
        dominated = False
        for j in idx:
            u, v = float(Y[j, 0]), float(Y[j, 1])
            if j != i and u >= a and v >= b and ((u, v) != (a, b) or j < i):
                dominated = True
                break
        if not dominated:
            pts.append((a, b))
    pts.sort()  # a ascending; b then descends
    out, prev = [], float(ref[0])
    for a, b in pts:
        out.append(((prev, float(ref[1])), (a, b)))
        prev = a
    return out


def _boxes3(Y, ref, idx):
    r0, r1, r2 = (float(v) for v in ref)
    order = sorted(idx, key=lambda i: (-float(Y[i, 2]), i))  # level order
    xs, nys, out = [], [], []  # the staircase of the points so far: y0 ascending, -y1 ascending
    for i in order:
        p0, p1, p2 = (float(v) for v in Y[i])
        t = len(xs)
        # strips i = first .. last (1-based, t + 1 the last strip): s_{i-1,0} < p0 and s_{i,1} < p1
        first = bisect.bisect_right(nys, -p1)  # 0-based staircase index of the first s with s_1 < p1
        stop = bisect.bisect_left(xs, p0)      # 0-based index of the first s with s_0 >= p0
        for k in range(first, min(stop, t - 1) + 1):
            left = r0 if k == 0 else xs[k - 1]
            right = min(xs[k], p0)
            floor = -nys[k]
            if left < right and floor < p1:
                out.append(((left, floor, r2), (right, p1, p2)))
        if stop >= t:  # the last strip: (s_t0, p0] x (ref_1, p1]
            left = r0 if t == 0 else xs[t - 1]
            if left < p0:
                out.append(((left, r1, r2), (p0, p1, p2)))
        # p joins the staircase unless an earlier point weakly dominates it in (y0, y1) (equal pairs: the first stays)
        if stop < t and -nys[stop] >= p1:
            continue
        start = bisect.bisect_left(nys, -p1)  # the points with s_0 <= p0 and s_1 <= p1 leave
        end = bisect.bisect_right(xs, p0)
        del xs[start:end], nys[start:end]
        xs.insert(start, p0)
        nys.insert(start, -p1)
    return out


def boxes(Y, ref):
    Y = np.asarray(Y, dtype=np.float64)
    m = Y.shape[1]
    idx = qualifying(Y, ref)
    if not idx:
        return np.zeros((0, m)), np.zeros((0, m))
    pairs = (_boxes1, _boxes2, _boxes3)[m - 1](Y, ref, idx)
    if not pairs:
        return np.zeros((0, m)), np.zeros((0, m))
    return np.array([p[0] for p in pairs], dtype=np.float64), np.array([p[1] for p in pairs], dtype=np.float64)


def padded(fronts, ref, J=None):
    """``bounds [S, 2, J, m]`` and ``count [S]`` for a list of sets; J defaults to the largest count (at least 1)."""
    per = [boxes(Y, ref) for Y in fronts]
    m = np.asarray(fronts[0]).shape[1]
    count = np.array([lo.shape[0] for lo, _ in per], dtype=np.int32)
    J = max(int(count.max()), 1) if J is None else J
    out = np.zeros((len(per), 2, J, m))
    for s, (lo, hi) in enumerate(per):
        out[s, 0, : lo.shape[0]], out[s, 1, : hi.shape[0]] = lo, hi
    return out, count


def count_bound(K, m):
    return 1 if m == 1 else (K if m == 2 else 2 * K - 1)


def volume_exact(lo, hi) -> Fraction:
    total = Fraction(0)
    for a, b in zip(lo, hi):
        v = Fraction(1)
        for x, y in zip(a, b):
            v *= Fraction(float(y)) - Fraction(float(x))
        total += v
    return total


def volume_fsum(lo, hi) -> float:
    return math.fsum(float(np.prod(b - a)) for a, b in zip(lo, hi))


def chain_length(K: int) -> int:
    """L of include/dkg.h: the longest chain of additions a term of dkg_hypervolume_front passes through."""
    return K + -(-K // 1024) + 10


def hv_bound(K: int, hv_ref: float) -> float:
    assert chain_length(K) <= K + 64
    return (chain_length(K) + 4) * EPS * hv_ref


def partition_defects(Y, ref, lo, hi):
    """Cells of the coordinate grid (all input values and ref, per axis) that lie in the wrong number of boxes:
    exactly one for a dominated cell, none otherwise.  Returns (cells checked, wrong cells)."""
    Y = np.asarray(Y, dtype=np.float64)
    m = Y.shape[1]
    q = qualifying(Y, ref)
    axes = [sorted(set([float(ref[c])] + [float(Y[i, c]) for i in q])) for c in range(m)]
    mids = [np.array([(a + b) / 2 for a, b in zip(ax[:-1], ax[1:])] + [ax[-1] + 1.0, ax[0] - 1.0]) for ax in axes]
    grid = np.stack(np.meshgrid(*mids, indexing="ij"), -1).reshape(-1, m)
    inside = np.zeros(grid.shape[0], dtype=np.int64)
    for a, b in zip(lo, hi):
        inside += ((grid > a) & (grid <= b)).all(-1)
    dominated = np.zeros(grid.shape[0], dtype=bool)
    for i in q:
        dominated |= ((grid > np.asarray(ref, dtype=np.float64)) & (grid <= Y[i])).all(-1)
    return grid.shape[0], int((inside != dominated.astype(np.int64)).sum())


def pairwise_disjoint(lo, hi, chunk=256) -> bool:
    """No two boxes (lo, hi] share interior."""
    n = lo.shape[0]
    for s in range(0, n, chunk):
        a_lo, a_hi = lo[s:s + chunk, None, :], hi[s:s + chunk, None, :]
        over = (np.maximum(a_lo, lo[None]) < np.minimum(a_hi, hi[None])).all(-1)
        over[np.arange(over.shape[0]), np.arange(s, s + over.shape[0])] = False
        if over.any():
            return False
    return True


def hi_dominated(Y, hi, chunk=256) -> bool:
    """Every upper corner is weakly dominated by a point."""
    Y = np.asarray(Y, dtype=np.float64)
    for s in range(0, hi.shape[0], chunk):
        if not (Y[None, :, :] >= hi[s:s + chunk, None, :]).all(-1).any(-1).all():
            return False
    return True


# ---- input cases -------------------------------------------------------------------------------------------------
KINDS = ("cloud", "front", "lattice", "equal", "ref")


def case(kind: str, K: int, m: int, seed: int = 0):
    """``(Y [K, m], ref [m])`` of one kind: a random cloud, a spherical front, a four-valued lattice (ties in every
    axis), all points equal, and a cloud with points on and below the reference point."""
    rng = np.random.default_rng(1000 * seed + 10 * K + m + 7 * KINDS.index(kind))
    ref = np.full(m, -0.25)
    if kind == "cloud":
        Y = rng.uniform(0.0, 1.0, (K, m))
    elif kind == "front":
        Y = np.abs(rng.normal(size=(K, m))) + 1e-3
        Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    elif kind == "lattice":
        Y = rng.integers(0, 4, (K, m)).astype(np.float64) / 4.0
    elif kind == "equal":
        Y = np.tile(rng.uniform(0.0, 1.0, (1, m)), (K, 1))
    else:
        Y = rng.uniform(0.0, 1.0, (K, m))
        ref = np.full(m, 0.3)
        for i in range(0, K, 3):
            Y[i, i % m] = 0.3  # on the reference point in one axis
        for i in range(1, K, 4):
            Y[i] = rng.uniform(-1.0, 0.2, m)  # below it
    return Y, ref


def antichain(n: int):
    """The lattice antichain {(i, j, n - 1 - i - j)} above ref (-1, -1, -1): n (n + 1) / 2 points, volume
    C(n + 2, 3), one box per point."""
    pts = [(i, j, n - 1 - i - j) for i in range(n) for j in range(n - i)]
    return np.array(pts, dtype=np.float64), np.full(3, -1.0)


def spherical_front(K: int, seed: int = 3):
    rng = np.random.default_rng(seed)
    Y = np.abs(rng.normal(size=(K, 3))) + 1e-3
    return Y / np.linalg.norm(Y, axis=1, keepdims=True), np.zeros(3)


def slab_boxes(Y, ref):
    """Another valid partition for m = 3, slab by slab on the last objective with the 2-d staircase boxes of the
    points reaching each slab (what slicing gives; many more boxes)."""
    Y = np.asarray(Y, dtype=np.float64)
    idx = qualifying(Y, ref)
    zs = sorted(set(float(Y[i, 2]) for i in idx), reverse=True)
    lo, hi = [], []
    for k, z in enumerate(zs):
        below = zs[k + 1] if k + 1 < len(zs) else float(ref[2])
        reach = [i for i in idx if Y[i, 2] >= z]
        for a, b in _boxes2(Y[:, :2], ref[:2], reach):
            lo.append(a + (below,))
            hi.append(b + (z,))
    return np.array(lo), np.array(hi)
