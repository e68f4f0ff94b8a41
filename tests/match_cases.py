"""Shared cases of the point-correspondence tests (csrc/match.hip): clouds by kind and (n, seed), the sizes, and brute(), the float64
numpy restatement of the nearest-neighbour definition of include/a3r.h.

Tie-free kinds (no two data points at the same distance from a query; the KD-tree route agrees with brute() on every index):
  uniform  g.uniform(-1, 1, (n, 3))
  range    g.standard_normal((n, 3)) * 10 ** g.uniform(-20, 18, (n, 1)): the squares overflow and underflow fp32 -- pins the float64
           arithmetic
  surface  a noisy height field seen through a pinhole: u = g.uniform(-1, 1, (n, 2)), z = 2 + 0.3 sin(3 u0) cos(2 u1) + 0.002 noise,
           points (u0 z, u1 z, z) -- what two overlapping views of a scene look like
Tie-rich kinds (exact ties everywhere; brute() is the only checker, a KD-tree returns some other index of the tie):
  lattice  g.integers(0, 6, (n, 3))
  offset   g.uniform(-1, 1, (n, 3)) * 0.01 + (1e4, -2e3, 5e3): the fp32 spacing there is about 1e-3, the points collapse onto a grid
           of duplicates -- pins direct differences (|a|^2 + |b|^2 - 2 a.b fails here)
P1 is drawn with seed 11, P2 with seed 12.
"""
import functools

import numpy as np

TIE_FREE = ("uniform", "range", "surface")
TIE_RICH = ("lattice", "offset")
KINDS = TIE_FREE + TIE_RICH
SIZES = [(1, 1), (3, 63), (65, 257), (1000, 1337), (4099, 5), (8193, 8191)]
SEED1, SEED2 = 11, 12


def cloud(kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == "uniform":
        p = g.uniform(-1, 1, (n, 3))
    elif kind == "range":
        p = g.standard_normal((n, 3)) * 10.0 ** g.uniform(-20, 18, (n, 1))
    elif kind == "surface":
        u = g.uniform(-1, 1, (n, 2))
        z = 2 + 0.3 * np.sin(3 * u[:, 0]) * np.cos(2 * u[:, 1]) + 0.002 * g.standard_normal(n)
        p = np.stack([u[:, 0] * z, u[:, 1] * z, z], 1)
    elif kind == "lattice":
        p = g.integers(0, 6, (n, 3))
    elif kind == "offset":
        p = g.uniform(-1, 1, (n, 3)) * 0.01 + np.array([1e4, -2e3, 5e3])
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p, dtype=np.float32).reshape(n, 3)


def pair(kind, n1, n2):
    return cloud(kind, n1, SEED1), cloud(kind, n2, SEED2)


def brute(Q, D, budget=1 << 21):
    """(index [nq] int32, d2 [nq] float64): for every query the smallest k with d2(q, k) = min over the finite d2, -1 and +inf where
    there is none.  d2 = dx*dx + dy*dy + dz*dz on float64 copies, evaluated in blocks of queries."""
    Q, D = np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(D, np.float32).astype(np.float64).reshape(-1, 3)
    nq, nd = len(Q), len(D)
    idx, best = np.full(nq, -1, np.int32), np.full(nq, np.inf)
    if nd == 0:
        return idx, best
    rows = max(1, budget // nd)
    with np.errstate(all="ignore"):
        for lo in range(0, nq, rows):
            q = Q[lo:lo + rows]
            dx, dy, dz = (q[:, None, c] - D[None, :, c] for c in range(3))
            d2 = dx * dx + dy * dy + dz * dz
            d2 = np.where(d2 < np.inf, d2, np.inf)              # NaN and +inf never win
            k = np.argmin(d2, 1)                                # the first minimum
            m = d2[np.arange(len(q)), k]
            idx[lo:lo + rows] = np.where(m < np.inf, k, -1)
            best[lo:lo + rows] = m
    return idx, best


def reciprocal(nn2_in_P1, nn1_in_P2):
    """(reciprocal_in_P2 [n2] bool, pairs [M,2] int32 (k1, k2) in ascending k2) from the two index arrays."""
    nn2, nn1 = np.asarray(nn2_in_P1), np.asarray(nn1_in_P2)
    k2 = np.arange(len(nn2))
    rec = np.zeros(len(nn2), bool)
    ok = nn2 >= 0
    rec[ok] = nn1[nn2[ok]] == k2[ok]
    return rec, np.stack([nn2[rec], k2[rec]], 1).astype(np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def brute_case(kind, n1, n2):
    """The restatement of a whole case, computed once per session: dict(P1, P2, nn2_in_P1, d2_2, nn1_in_P2, d2_1, reciprocal_in_P2,
    pairs).  Callers leave the arrays unchanged."""
    P1, P2 = pair(kind, n1, n2)
    nn2, d22 = brute(P2, P1)
    nn1, d21 = brute(P1, P2)
    rec, pairs = reciprocal(nn2, nn1)
    out = dict(P1=P1, P2=P2, nn2_in_P1=nn2, d2_2=d22, nn1_in_P2=nn1, d2_1=d21, reciprocal_in_P2=rec, pairs=pairs)
    for v in out.values():
        v.setflags(write=False)
    return out
