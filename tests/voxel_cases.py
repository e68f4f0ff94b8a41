"""Shared cases of the voxel-grid tests (csrc/voxel.hip): voxel_ref(), the numpy restatement of the definition in include/a3r.h, a slow
dict-of-lists checker of it, and the clouds by kind.

The definition, on float64 copies of the fp32 inputs, every operation rounded on its own:
    r = x / voxel, q = floor(r) per coordinate; in a voxel iff the coordinates are finite and -2^20 <= q < 2^20 for all three
    key = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20)
    value = (w << 32) | row; w = 0 without priorities, else ~(b ^ (0xffffffff if b >> 31 else 0x80000000)) of the fp32 bits b, all
    ones for a NaN; the winner of a voxel is its minimum value, count the number of its points; kept iff count >= min_count; the
    output is in ascending winner row
    best: the winner's rows.  mean: t = uint64(floor((r - q) * 2^24)), S = sum t, ((q + (S + 0.5 n) / (n 2^24)) * voxel) as float32;
    colours (2 sum + n) // (2 n)

Kinds (cloud(kind, M, k) -> xyz [M,3] float32, voxel, priority [M] float32, rgb [M,3] uint8):
  surface    (u, v, 0.3 sin 3u cos 2v + noise) on [-1,1]^2, priorities in [1,10], voxel = 2 sqrt(4k / M): no power of two, so the
             quotient's rounding matters; from M = 65 up a case keeps 0.05 <= V/M <= 0.5 and a largest count >= 5
  ties       the surface with priorities drawn from three values: exact ties in almost every voxel
  nan_prio   the surface with a tenth of the priorities NaN, and five more points in a voxel of their own whose priorities are all NaN
  runs       the surface sorted by cell, a fiftieth of the rows made NaN in one coordinate: neighbouring rows share a cell in runs of
             every length, across wave and workgroup borders, interrupted by dropped rows (the insert pass folds such runs)
  pile       all M points in one voxel, equal priorities: V = 1, count = M, winner row 0 -- the maximal contention on one slot
  pile_prio  the same with distinct priorities, the largest at the last row (the last workgroup)
  spread     lattice points, one per voxel, in shuffled order: V = M, every count 1, index = arange(M)
  edges      the nine boundary rows of the issue at voxel = 0.25: -0.0, exact cell borders, +-1e-30, NaN, inf, the last cell inside
             +-2^20 and the first outside
  edges_rep  those rows three times over plus interior points of the two outermost cells: boundary points share voxels
  empty      M = 0
"""
import functools
import math

import numpy as np

R = 1 << 20
FIX = float(1 << 24)
SIZES = [63, 64, 65, 1025, 8193, 70001]

CASES = [("empty", 0, 1), ("edges", 9, 1), ("edges_rep", 31, 1)]
for _M in SIZES:
    CASES += [("surface", _M, 1), ("surface", _M, 4), ("ties", _M, 1), ("nan_prio", _M + 5, 4), ("runs", _M, 4)]
for _M in [1] + SIZES:
    CASES += [("pile", _M, 1), ("pile_prio", _M, 1), ("spread", _M, 1)]


def case_id(case):
    return f"{case[0]}-M{case[1]}-k{case[2]}"


# ------------------------------------------------------------------------------------------------- the restatement
def voxel_cells(xyz, voxel):
    """(inside [M] bool, key [M] uint64 (0 where not inside), r [M,3], q [M,3] float64)."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        r = x / np.float64(voxel)
        q = np.floor(r)
        inside = (np.isfinite(x) & (q >= -R) & (q < R)).all(1)
    qi = (np.where(inside[:, None], q, 0.0) + R).astype(np.uint64)
    key = (qi[:, 0] << np.uint64(42)) | (qi[:, 1] << np.uint64(21)) | qi[:, 2]
    return inside, key, r, q


def priority_words(priority, M):
    """w [M] uint64: the larger priority has the smaller word, NaN the largest; zeros without priorities."""
    if priority is None:
        return np.zeros(M, np.uint64)
    p = np.ascontiguousarray(priority, np.float32).reshape(M)
    b = p.view(np.uint32)
    w = ~(b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)))
    return np.where(np.isnan(p), np.uint32(0xFFFFFFFF), w).astype(np.uint64)


def voxel_ref(xyz, voxel, priority=None, rgb=None, reduce="best", min_count=1):
    """The restatement: dict(xyz [V,3] float32, rgb [V,3] uint8 or None, index [V] int32, count [V] int32, dropped int)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    M = len(xyz)
    inside, key, r, q = voxel_cells(xyz, voxel)
    rows = np.flatnonzero(inside)
    uniq, inv, counts = np.unique(key[rows], return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    value = (priority_words(priority, M)[rows] << np.uint64(32)) | rows.astype(np.uint64)
    best = np.full(len(uniq), 0xFFFFFFFFFFFFFFFF, np.uint64)
    np.minimum.at(best, inv, value)
    winner = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = np.flatnonzero(counts >= min_count)
    ids = ids[np.argsort(winner[ids], kind="stable")]
    index, n = winner[ids], counts[ids].astype(np.int64)
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    if reduce == "best":
        out_xyz, out_rgb = xyz[index], (rgb[index] if rgb is not None else None)
    elif reduce == "mean":
        t = np.floor((r[rows] - q[rows]) * FIX).astype(np.uint64)
        S = np.zeros((len(uniq), 3), np.uint64)
        np.add.at(S, inv, t)
        nd = n.astype(np.float64)[:, None]
        out_xyz = ((q[index] + (S[ids].astype(np.float64) + 0.5 * nd) / (nd * FIX)) * np.float64(voxel)).astype(np.float32)
        out_rgb = None
        if rgb is not None:
            Csum = np.zeros((len(uniq), 3), np.uint64)
            np.add.at(Csum, inv, rgb[rows].astype(np.uint64))
            nu = n.astype(np.uint64)[:, None]
            out_rgb = ((np.uint64(2) * Csum[ids] + nu) // (np.uint64(2) * nu)).astype(np.uint8)
    else:
        raise ValueError(reduce)
    return dict(xyz=np.ascontiguousarray(out_xyz.reshape(-1, 3)), rgb=None if out_rgb is None else np.ascontiguousarray(out_rgb.reshape(-1, 3)),
                index=index.astype(np.int32), count=n.astype(np.int32), dropped=int(M - len(rows)))


def voxel_naive(xyz, voxel, priority=None, rgb=None, reduce="best", min_count=1):
    """The definition once more, point by point in plain Python with a dict of lists (the checker of voxel_ref on the small sizes)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cells, dropped = {}, 0
    for i, p in enumerate(xyz):
        qs, ts = [], []
        for a in range(3):
            x = float(p[a])
            if not math.isfinite(x):
                break
            rr = x / float(voxel)
            if not math.isfinite(rr):
                break
            qq = math.floor(rr)
            if not -R <= qq < R:
                break
            qs.append(qq)
            ts.append(math.floor((rr - qq) * FIX))
        if len(qs) < 3:
            dropped += 1
            continue
        cells.setdefault(tuple(qs), []).append((i, ts))

    def beats(i, j):                   # does row i win against row j?  (i != j)
        if priority is None:
            return i < j
        a, b = np.float32(priority[i]), np.float32(priority[j])
        if np.isnan(a) or np.isnan(b):
            return (not np.isnan(a)) if np.isnan(a) != np.isnan(b) else i < j
        ka, kb = (float(a), not np.signbit(a)), (float(b), not np.signbit(b))       # +0 ranks above -0, as the bit order has it
        return ka > kb if ka != kb else i < j

    out = []
    for qs, pts in cells.items():
        if len(pts) < min_count:
            continue
        win = pts[0][0]
        for i, _ in pts[1:]:
            if beats(i, win):
                win = i
        n = len(pts)
        if reduce == "best":
            pos, col = xyz[win], (rgb[win] if rgb is not None else None)
        else:
            pos = [np.float32((float(qs[a]) + (float(sum(t[a] for _, t in pts)) + 0.5 * n) / (float(n) * FIX)) * float(voxel)) for a in range(3)]
            col = [(2 * sum(int(rgb[i][c]) for i, _ in pts) + n) // (2 * n) for c in range(3)] if rgb is not None else None
        out.append((win, n, pos, col))
    out.sort(key=lambda e: e[0])
    return dict(xyz=np.array([e[2] for e in out], np.float32).reshape(-1, 3),
                rgb=None if rgb is None else np.array([e[3] for e in out], np.uint8).reshape(-1, 3),
                index=np.array([e[0] for e in out], np.int32), count=np.array([e[1] for e in out], np.int32), dropped=dropped)


# ------------------------------------------------------------------------------------------------- the clouds
EDGE_VOXEL = 0.25
EDGE_ROWS = np.array([[-0.0, 0, 0.25], [-0.25, 0.25, -0.5], [-1e-30, 1e-30, 0.5], [np.nan, 0, 0], [np.inf, 0, 0], [0.25 * (R - 1), 0, 0],
                      [0.25 * R, 0, 0], [-0.25 * R, 0, 0], [-0.25 * R - 0.1, 0, 0]], np.float32)
EDGE_WINNERS, EDGE_DROPPED = [0, 1, 2, 5, 7], 4


def surface_voxel(M, k):
    return 2.0 * math.sqrt(4.0 * k / M)


def _surface(g, M):
    u, v = g.uniform(-1, 1, M), g.uniform(-1, 1, M)
    return np.stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.002 * g.standard_normal(M)], 1).astype(np.float32)


def colours(M, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (M, 3), dtype=np.uint8)


def cloud(kind, M, k=1):
    """(xyz [M,3] float32, voxel, priority [M] float32, rgb [M,3] uint8) of a case."""
    g = np.random.default_rng(100 + 7 * M + k)
    rgb = colours(M, 3 + M)
    if kind == "empty":
        assert M == 0
        return np.zeros((0, 3), np.float32), 0.5, np.zeros(0, np.float32), rgb
    if kind == "surface":
        return _surface(g, M), surface_voxel(M, k), g.uniform(1, 10, M).astype(np.float32), rgb
    if kind == "ties":
        return _surface(g, M), surface_voxel(M, k), g.choice(np.array([1.0, 2.5, 7.0], np.float32), M), rgb
    if kind == "runs":
        xyz, voxel = _surface(g, M), surface_voxel(M, k)
        xyz = xyz[np.argsort(voxel_cells(xyz, voxel)[1], kind="stable")]
        bad = g.permutation(M)[:max(M // 50, 1)]
        xyz[bad, g.integers(0, 3, len(bad))] = np.nan
        return xyz, voxel, g.uniform(1, 10, M).astype(np.float32), rgb
    if kind == "nan_prio":
        xyz = _surface(g, M)
        pr = g.uniform(1, 10, M).astype(np.float32)
        pr[g.random(M) < 0.1] = np.nan
        xyz[-5:] = np.float32(5.0) + (0.01 * g.random((5, 3))).astype(np.float32)      # far from the surface: voxels that hold NaN priorities only
        pr[-5:] = np.nan
        return xyz, surface_voxel(M - 5, k), pr, rgb
    if kind in ("pile", "pile_prio"):
        voxel = 0.37
        xyz = (voxel * (np.array([3.0, -2.0, 5.0]) + g.uniform(0.1, 0.9, (M, 3)))).astype(np.float32)
        if kind == "pile":
            return xyz, voxel, np.full(M, 2.5, np.float32), rgb
        pr = g.permutation(M).astype(np.float32)
        top, at = int(np.argmax(pr)), M - 1
        pr[[top, at]] = pr[[at, top]]
        return xyz, voxel, pr, rgb
    if kind == "spread":
        side = 47
        assert M <= side ** 3
        cell = g.permutation(side ** 3)[:M]
        lat = np.stack([cell % side, (cell // side) % side, cell // (side * side)], 1) - side // 2
        return ((lat + 0.25) * 0.5).astype(np.float32), 0.5, g.uniform(1, 10, M).astype(np.float32), rgb
    if kind == "edges":
        assert M == len(EDGE_ROWS)
        return EDGE_ROWS.copy(), EDGE_VOXEL, g.uniform(1, 10, M).astype(np.float32), rgb
    if kind == "edges_rep":
        inner = np.array([[0.25 * (R - 1) + 0.125, 0.125, 0.125], [-0.25 * R + 0.125, 0.125, 0.125]], np.float32)
        xyz = np.concatenate([EDGE_ROWS, inner, EDGE_ROWS, inner, EDGE_ROWS])
        assert M == len(xyz)
        return xyz, EDGE_VOXEL, g.uniform(1, 10, M).astype(np.float32), rgb
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def ref_case(case):
    """A whole case, computed once per session: dict(xyz, voxel, priority, rgb, best, mean) with best / mean the restatement's dicts
    at min_count = 1.  Callers leave the arrays unchanged."""
    kind, M, k = case
    xyz, voxel, priority, rgb = cloud(kind, M, k)
    out = dict(xyz=xyz, voxel=voxel, priority=priority, rgb=rgb)
    for reduce in ("best", "mean"):
        out[reduce] = voxel_ref(xyz, voxel, priority, rgb, reduce, 1)
    for a in [xyz, priority, rgb] + [v for r in ("best", "mean") for v in out[r].values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return out
