"""Host side of the flow-kernel pins (tests/test_gpu_flow_kernels_f64.py, tests/test_flow_refs_cpu.py): seeded inputs, float64
references, numpy fp32 restatements of the kernels' arithmetic order (csrc/raft.hip), and the tolerances.  No GPU, no library call.

The float64 references are written from the formulas the kernel comments cite in the reference (corr.py:22,25-50, utils.py:76-91,
raft.py:183-199, layer.py:125) with torch's own float64 conv2d, grid_sample(align_corners=True), interpolate, unfold and softmax.
Every tolerance is derived from the number format and the operation count, never from what a kernel returns; U = 2^-24 is the
relative error of one fp32 rounding.  The restatements exist so that the CPU test can show that fp32 arithmetic in the kernels'
order uses at most half of each tolerance: what the GPU test then catches is a kernel that computes something else."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
U = 2.0 ** -24
CAP = 1 << 24            # grid1d caps a launch at 65536 workgroups of 256 threads: work item CAP + i is thread i's second trip
# Allowance for the device's expf against numpy's, in ulps of the result: the HIP math API documents a maximum error of 1 ulp for expf
# (ROCm "HIP math API", single precision table); the restatement rounds a float64 exp (half an ulp).  2 leaves the device twice its bound.
EXPF_ULPS = 2.0


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _fma32(a, b, c):
    """fmaf of fp32 operands: the product is exact in float64, one rounding of the sum to fp32 (up to a double rounding)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def cap_items(total):
    """The work items of a past-the-cap case that get a float64 reference: the first and the last, and 256 on each side of every
    multiple of CAP below the total."""
    assert total > CAP
    it = [np.array([0, total - 1])]
    for m in range(CAP, total, CAP):
        it.append(np.arange(m - 256, min(m + 256, total)))
    return np.unique(np.concatenate(it))


# ------------------------------------------------------------------------------------------------------------ 7x7 direct convolutions
IN_MUL, IN_ADD = F32(2.0 / 255.0), F32(-1.0)               # raft.py:194-195
# (H, W, two sources, Cout, B, relu): every shape with one and two sources, both widths, both batch sizes, relu on and off.
# Wo = 4, 20, 8, 28: Wo % 8 = 4 (the last thread of a row owns half its columns) and 0; 8x8 is smaller than the filter's reach
STEM_SHAPES = [(8, 8), (24, 40), (16, 16), (40, 56)]
STEM_CASES = [(H, W, two, Cout, B, relu) for H, W in STEM_SHAPES
              for two, Cout, B, relu in ((False, 32, 1, True), (True, 64, 2, False), (False, 64, 2, True), (True, 32, 1, False))]
# (h, w, Cout, relu) on the channels-last coarse flow, B = 2: w % 8 = 2, 7, 4, 5
CONVF_CASES = [(h, w, Cout, relu) for h, w in ((2, 2), (5, 7), (16, 20), (22, 21)) for Cout, relu in ((64, True), (128, False))]
FLOW_MAX = 100.0


def stem_inputs(H, W, two, Cout, B, seed):
    """x0, x1 (or None) [B, 3, H, W] in [0, 255]; w [Cout, Cin, 7, 7]; bias [Cout]"""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(0, 255, (B, 3, H, W)).astype(F32)
    x1 = rng.uniform(0, 255, (B, 3, H, W)).astype(F32) if two else None
    w = (0.1 * rng.standard_normal((Cout, 6 if two else 3, 7, 7))).astype(F32)
    b = (0.5 * rng.standard_normal(Cout)).astype(F32)
    return x0, x1, w, b


def convf_inputs(h, w, Cout, seed, B=2):
    """flow [B, h, w, 2] with |values| up to FLOW_MAX (the extremes present); w [Cout, 2, 7, 7]; bias [Cout]"""
    rng = np.random.default_rng(seed)
    flow = rng.uniform(-FLOW_MAX, FLOW_MAX, (B, h, w, 2)).astype(F32)
    flow.reshape(-1)[[0, -1]] = (FLOW_MAX, -FLOW_MAX)
    wt = (0.02 * rng.standard_normal((Cout, 2, 7, 7))).astype(F32)
    b = (2.0 * rng.standard_normal(Cout)).astype(F32)
    return flow, wt, b


def stem_planes(x0, x1):
    return x0 if x1 is None else np.concatenate([x0, x1], axis=1)


def conv7_ref64(x, w, b, stride, relu, in_mul=1.0, in_add=0.0):
    """x [B, Cin, H, W] fp32 planes -> (y float64 [B, Ho, Wo, Cout], tolerance of the same shape).  The input enters as
    x^ = x in_mul + in_add; padding pads x^ with zeros.
    Tolerance: a chain of n fused multiply-adds started at the bias has error <= (n + 2) U (sum |x^| |w| + |b|), n the taps inside the
    image (conv of ones); the normalisation, x^ = fl(fl(x in_mul) + in_add) or one fma, adds |dx^| <= U (|x in_mul| + |x^|) per tap
    (nothing when in_mul = 1, in_add = 0: then x^ = x exactly).  relu is 1-Lipschitz."""
    x64 = _t64(x)
    xh = x64 * float(in_mul) + float(in_add)
    w64, b64 = _t64(w), _t64(b)
    y = F.conv2d(xh, w64, b64, stride=stride, padding=3)
    if relu:
        y = y.relu()
    n = F.conv2d(torch.ones(1, 1, *x.shape[2:], dtype=torch.float64), torch.ones(1, 1, 7, 7, dtype=torch.float64), stride=stride, padding=3) * x.shape[1]
    s = F.conv2d(xh.abs(), w64.abs(), stride=stride, padding=3) + b64.abs()[None, :, None, None]
    tol = (n + 2) * U * s
    if not (float(in_mul) == 1.0 and float(in_add) == 0.0):
        tol = tol + U * F.conv2d((x64 * float(in_mul)).abs() + xh.abs(), w64.abs(), stride=stride, padding=3)
    return y.permute(0, 2, 3, 1).numpy(), tol.permute(0, 2, 3, 1).numpy()


def conv7_restated(x, w, b, stride, relu, in_mul=F32(1), in_add=F32(0)):
    """direct_conv_fixed_kernel / direct_conv_kernel in numpy fp32: acc = bias; for c, ky, kx: acc = fma(x^, w, acc); zeros outside"""
    B, Cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xh = (x * F32(in_mul)).astype(F32) + F32(in_add)
    xp = np.zeros((B, Cin, H + 6 + stride, W + 6 + stride), F32)
    xp[:, :, 3:3 + H, 3:3 + W] = xh
    acc = np.broadcast_to(b.astype(F32), (B, Ho, Wo, w.shape[0])).copy()
    for c in range(Cin):
        for ky in range(7):
            for kx in range(7):
                patch = xp[:, c, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]
                acc = _fma32(patch[..., None], w[:, c, ky, kx][None, None, None, :], acc)
    return np.maximum(acc, F32(0)) if relu else acc


# past the cap: B Ho ceil(Wo / 8) Cout > 2^24 -- what the stems of 48 pairs of 384 x 512 run (48 x 192 x 32 x 64 = 18.9 M threads).
# One 2048 x 4112 frame, Cout = 64: 1024 x 257 x 64 = 2^24 + 65536 threads, Wo = 2056 (% 8 = 0), the smallest such width at this height
STEM_CAP = (1, 2048, 4112, 64)


def stem_items(shape_out, items):
    """work item i of direct_conv_fixed_kernel<7, 2, 8> -> (b, oy, column group, co); shape_out = (B, Ho, Wo, Cout)"""
    B, Ho, Wo, Cout = shape_out
    WoG = (Wo + 7) // 8
    co, p = items % Cout, items // Cout
    g, p = p % WoG, p // WoG
    return p // Ho, p % Ho, g, co


def stem_ref64_at(slab, w, b, H, W, items, relu, in_mul, in_add):
    """float64 stem outputs (stride 2) of the given work items of a [B, Cin, H, W] call: (rows [n] of (b, oy, ox, co), y [n], tol [n]).
    slab(b, y0, y1, x0, x1) -> x[b, :, y0:y1, x0:x1] as a numpy array.  Per (b, oy, group): the 7 x 21 patch of x^ its 8 columns read,
    zeros outside the image, through an unpadded conv2d; the tolerance is conv7_ref64's with n = 49 Cin taps (an upper count)."""
    Cout, Cin = w.shape[:2]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ib, iy, ig, ic = stem_items((None, Ho, Wo, Cout), items)
    w64, b64 = _t64(w), _t64(b)
    rows, ys, tols = [], [], []
    for kb, ky, kg in sorted(set(zip(ib.tolist(), iy.tolist(), ig.tolist()))):
        cs = np.unique(ic[(ib == kb) & (iy == ky) & (ig == kg)])
        ty, tx = 2 * ky - 3, 16 * kg - 3
        y0, y1, x0, x1 = max(ty, 0), min(ty + 7, H), max(tx, 0), min(tx + 21, W)
        x64 = _t64(slab(kb, y0, y1, x0, x1))
        xh, xm = torch.zeros(1, Cin, 7, 21, dtype=torch.float64), torch.zeros(1, Cin, 7, 21, dtype=torch.float64)
        xh[0, :, y0 - ty:y1 - ty, x0 - tx:x1 - tx] = x64 * float(in_mul) + float(in_add)
        xm[0, :, y0 - ty:y1 - ty, x0 - tx:x1 - tx] = (x64 * float(in_mul)).abs()
        yy = F.conv2d(xh, w64, b64, stride=2)[0, :, 0]                               # [Cout, 8]
        tt = (49 * Cin + 2) * U * (F.conv2d(xh.abs(), w64.abs(), stride=2)[0, :, 0] + b64.abs()[:, None]) \
            + U * F.conv2d(xm + xh.abs(), w64.abs(), stride=2)[0, :, 0]
        if relu:
            yy = yy.relu()
        for q in range(8):
            if 8 * kg + q >= Wo:
                continue
            for c in cs:
                rows.append((kb, ky, 8 * kg + q, int(c)))
                ys.append(float(yy[c, q]))
                tols.append(float(tt[c, q]))
    return np.array(rows), np.array(ys), np.array(tols)


# ------------------------------------------------------------------------------------------------------------ depthwise 7x7
# (h, w, C) at B = 2: w % 4 = 1, 1, 0, 1, 2; h < 7 in three of them
DW_CASES = [(h, w, C) for h, w in ((1, 1), (3, 5), (16, 20), (22, 21), (9, 42)) for C in (192, 384)]
DW_CAP = (16, 64, 172, 384)         # the smallest B x h x w of this family at C = 384 with B h ceil(w / 4) C > 2^24 (15 x 64 x 172: 15.9 M)


def dw_inputs(h, w, C, seed, B=2):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, h, w, C)).astype(F32)
    wt = (0.2 * rng.standard_normal((C, 49))).astype(F32)
    b = rng.standard_normal(C).astype(F32)
    return x, wt, b


def dw_ref64(x, w, b):
    """x [B, h, w, C] channels-last, w [C, 49], b [C] -> (y float64, tolerance (n + 2) U (sum |x| |w| + |b|), n the taps inside)"""
    C = x.shape[-1]
    x64, w64, b64 = _t64(x).permute(0, 3, 1, 2), _t64(w).view(C, 1, 7, 7), _t64(b)
    y = F.conv2d(x64, w64, b64, padding=3, groups=C)
    n = F.conv2d(torch.ones(1, 1, *x.shape[1:3], dtype=torch.float64), torch.ones(1, 1, 7, 7, dtype=torch.float64), padding=3)
    s = F.conv2d(x64.abs(), w64.abs(), padding=3, groups=C) + b64.abs()[None, :, None, None]
    return y.permute(0, 2, 3, 1).numpy(), ((n + 2) * U * s).permute(0, 2, 3, 1).numpy()


def dw_restated(x, w, b):
    """dwconv7_kernel in numpy fp32: acc = bias; for ky, kx: acc = fma(x, w[ky 7 + kx], acc) over the taps inside"""
    B, h, wd, C = x.shape
    xp = np.zeros((B, h + 6, wd + 6, C), F32)
    xp[:, 3:3 + h, 3:3 + wd] = x
    acc = np.broadcast_to(b.astype(F32), x.shape).copy()
    for ky in range(7):
        for kx in range(7):
            acc = _fma32(xp[:, ky:ky + h, kx:kx + wd], w[:, ky * 7 + kx], acc)
    return acc


def dw_items(shape, items):
    """work item i of dwconv7_kernel's loop -> (b, oy, column group, c)"""
    B, h, w, C = shape
    wG = (w + 3) // 4
    c, p = items % C, items // C
    g, p = p % wG, p // wG
    return p // h, p % h, g, c


def dw_ref64_at(slab, w, b, shape, items):
    """float64 depthwise outputs of the given work items: (rows [n] of (b, oy, ox, c), y [n], tol [n]); an item owns up to 4 columns.
    slab(b, y0, y1, x0, x1) -> x[b, y0:y1, x0:x1, :] as a numpy array (the caller's array may live on a device)."""
    B, h, wd, C = shape
    ib, iy, ig, ic = dw_items(shape, items)
    rows, ys, tols = [], [], []
    for kb, ky, kg in sorted(set(zip(ib.tolist(), iy.tolist(), ig.tolist()))):
        cs = np.unique(ic[(ib == kb) & (iy == ky) & (ig == kg)])
        y0, y1, x0, x1 = max(ky - 3, 0), min(ky + 4, h), max(4 * kg - 3, 0), min(4 * kg + 7, wd)
        patch = np.zeros((1, 7, 10, C), F32)
        patch[0, y0 - (ky - 3):y1 - (ky - 3), x0 - (4 * kg - 3):x1 - (4 * kg - 3)] = slab(kb, y0, y1, x0, x1)
        # the 7 x 10 patch, zero outside the map, as a 7-row map whose row 3 holds the item's outputs at columns 3..6
        yy, tt = dw_ref64(patch, w, b)
        # (the tolerance counts the patch's 49 taps where the map may have fewer inside: (n + 2) with n = 49 bounds every chain)
        for q in range(4):
            if 4 * kg + q >= wd:
                continue
            for c in cs:
                rows.append((kb, ky, 4 * kg + q, int(c)))
                ys.append(yy[0, 3, 3 + q, c])
                tols.append(tt[0, 3, 3 + q, c])
    return np.array(rows), np.array(ys), np.array(tols)


# ------------------------------------------------------------------------------------------------------------ gather_s2, halve
GH_CASES = [(h, w, C) for h, w in ((2, 2), (5, 5), (22, 21), (9, 7)) for C in (128, 256)]


# past the cap: B ho wo C / 4 > 2^24 -- what the feature network's first strided block runs on the 96 frames of 48 pairs of 384 x 512
# (96 x 96 x 128 x 16 = 18.9 M threads).  257 x 129 x 8 output pixels of 256 channels: 2^24 + 196608 threads
GATHER_CAP = (8, 513, 257, 256)


def gh_input(h, w, C, seed, B=2):
    return np.random.default_rng(seed).standard_normal((B, h, w, C)).astype(F32) * F32(3)


def gather_ref(x):
    """the sampling of a 1x1 convolution with stride 2 (layer.py:125): x[:, ::2, ::2]"""
    k = torch.zeros(1, 1, 1, 1, dtype=torch.float64) + 1
    B, h, w, C = x.shape
    y = F.conv2d(_t64(x).permute(0, 3, 1, 2).reshape(B * C, 1, h, w), k, stride=2)
    return y.reshape(B, C, *y.shape[2:]).permute(0, 2, 3, 1).numpy()


def halve_ref64(x):
    """F.interpolate(scale_factor=0.5, mode='bilinear', align_corners=False) (corr.py:22) -> (y float64, tolerance).
    Worst case: t0 = fl(.5 a + .5 b), t1 likewise, y = fl(.5 t0 + .5 t1): three roundings, each of a value <= max |block|, two of
    them entering halved, so |error| <= 2 U max |block|.  That bound is attainable in fp32, so the tolerance is twice it, 4 U max
    |block| (2^-22 max |block|): fp32 in this order then provably uses at most half."""
    y = F.interpolate(_t64(x).permute(0, 3, 1, 2), scale_factor=0.5, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    ho, wo = y.shape[1:3]
    a = np.abs(x[:, :2 * ho, :2 * wo].astype(np.float64)).reshape(x.shape[0], ho, 2, wo, 2, x.shape[3])
    return y, 4 * U * a.max(axis=(2, 4))


def halve_restated(x):
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    v = x[:, :2 * ho, :2 * wo]
    h5 = F32(0.5)
    t0 = h5 * v[:, 0::2, 0::2] + h5 * v[:, 0::2, 1::2]
    t1 = h5 * v[:, 1::2, 0::2] + h5 * v[:, 1::2, 1::2]
    return h5 * t0 + h5 * t1


# ------------------------------------------------------------------------------------------------------------ correlation lookup
LK_FAMILIES = ("inside", "integral", "border", "exact", "outside")
LK_CONFIGS = [(2, 4), (4, 4), (4, 2)]                       # (r, levels)
LK_MAPS = [(16, 20), (22, 21)]                              # pyramids 16x20, 8x10, 4x5, 2x2 and 22x21, 11x10, 5x5, 2x2
LK_CAP = (187, 16, 16, 4, 4, 352)                           # B, h, w, r, levels, ldo: 187 x 256 x 352 > 2^24 >= 186 x 256 x 352


def lk_levels(h, w, levels):
    return [(h >> l, w >> l) for l in range(levels)]


def lk_ldos(r, levels):
    """ldo of the three calls of a case: the channel count, one above it, padded to 32"""
    n = levels * (2 * r + 1) ** 2
    return [n, n + 1, (n + 31) // 32 * 32 if n % 32 else n + 32]


def lk_inputs(h, w, r, levels, seed, B=2):
    """corr: per level [B h w, h_l, w_l], drawn independently for every query; qx, qy [Q]; flow [Q, 2] fp32; fam [Q].
    Families (a seeded permutation spreads them over the map): targets inside the map of every level; exactly integral targets; targets within one
    pixel either side of a border of a level (level and side drawn per query); targets exactly at -1 or at W_l / H_l of a level; and
    targets whose whole window lies outside the map at every level."""
    rng = np.random.default_rng(seed)
    Q = B * h * w
    sizes = lk_levels(h, w, levels)
    corr = [rng.standard_normal((Q, hl, wl)).astype(F32) for hl, wl in sizes]
    q = np.arange(Q)
    qx, qy = q % w, (q // w) % h
    fam = rng.permutation(Q) % len(LK_FAMILIES)
    in_x, in_y = min((wl - 1) << l for l, (hl, wl) in enumerate(sizes)), min((hl - 1) << l for l, (hl, wl) in enumerate(sizes))
    tx, ty = rng.uniform(0, in_x, Q), rng.uniform(0, in_y, Q)                     # inside the map at EVERY level (a level floors its size)
    k = fam == 1
    tx[k], ty[k] = rng.integers(0, w, k.sum()), rng.integers(0, h, k.sum())
    lv, side = rng.integers(0, levels, Q), rng.integers(0, 4, Q)
    hl, wl = np.array([s[0] for s in sizes])[lv], np.array([s[1] for s in sizes])[lv]
    s2 = 2.0 ** lv
    near = rng.uniform(-1, 1, Q)
    for f, lo_x, hi_x, lo_y, hi_y in ((2, near * s2, (wl - 1 + near) * s2, near * s2, (hl - 1 + near) * s2),
                                      (3, -s2, wl * s2, -s2, hl * s2)):
        for sd, axis, val in ((0, 0, lo_x), (1, 0, hi_x), (2, 1, lo_y), (3, 1, hi_y)):
            k = (fam == f) & (side == sd)
            (tx if axis == 0 else ty)[k] = val[k]
    far = (r + 2) * 2.0 ** (levels - 1) + rng.uniform(0, 10, Q)
    for sd, axis, val in ((0, 0, -far), (1, 0, w + far), (2, 1, -far), (3, 1, h + far)):
        k = (fam == 4) & (side == sd)
        (tx if axis == 0 else ty)[k] = val[k]
    flow = np.stack([tx - qx, ty - qy], axis=1).astype(F32)
    return corr, qx, qy, flow, fam


def _taps64(c, yy, xx):
    """c [n, H, W]; integer yy, xx [n, ...] -> c[q, yy, xx], zero outside"""
    n, H, W = c.shape
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    qi = np.arange(n).reshape((n,) + (1,) * (yy.ndim - 1))
    return np.where(ok, c[qi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0)


def _lk_positions(qx, qy, flow, l, r):
    """float64 sampling positions [n, win, win] of level l: the FIRST window index moves x (corr.py:37-43 stacks meshgrid(dy, dx))"""
    d = np.arange(-r, r + 1, dtype=np.float64)
    cx, cy = qx + flow[:, 0].astype(np.float64), qy + flow[:, 1].astype(np.float64)
    px = (cx / 2 ** l)[:, None, None] + d[None, :, None] + 0 * d[None, None, :]
    py = (cy / 2 ** l)[:, None, None] + d[None, None, :] + 0 * d[None, :, None]
    return cx, cy, px, py


def lookup_ref64(corr, qx, qy, flow, r, route="grid_sample"):
    """out float64 [n, levels (2r+1)^2].  route 'grid_sample': bilinear_sampler (utils.py:76-91) -- normalise, then
    F.grid_sample(align_corners=True); route 'explicit': floor and the four weights, zeros outside."""
    out = []
    for l, c in enumerate(corr):
        n, H, W = c.shape
        _, _, px, py = _lk_positions(qx, qy, flow, l, r)
        if route == "grid_sample":
            grid = torch.from_numpy(np.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], axis=-1))
            s = F.grid_sample(_t64(c)[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0].numpy()
        else:
            x0, y0 = np.floor(px), np.floor(py)
            wx, wy = px - x0, py - y0
            x0, y0, c64 = x0.astype(np.int64), y0.astype(np.int64), c.astype(np.float64)
            s = (_taps64(c64, y0, x0) * (1 - wx) * (1 - wy) + _taps64(c64, y0, x0 + 1) * wx * (1 - wy)
                 + _taps64(c64, y0 + 1, x0) * (1 - wx) * wy + _taps64(c64, y0 + 1, x0 + 1) * wx * wy)
        out.append(s.reshape(n, -1))
    return np.concatenate(out, axis=1)


def lookup_tol(corr, qx, qy, flow, r):
    """[n, levels (2r+1)^2].  Bilinear sampling with zero padding is continuous and piecewise linear, so the error has two parts.
    Coordinates, per axis (W the level's size, c = x + flow, p the position): c = fl(x + f): U |c|, halved l times exactly;
    p = fl(c / 2^l + offset): U |p|; 2 p / (W - 1): U |that|, - 1: U |g|, back: g + 1: U |g + 1|, times (W - 1): U |ix| -- five
    roundings after the first, in pixels U (|p| + |p| + |p - (W - 1) / 2| + |p| + |p|) <= U (5 |p| + (W - 1) / 2).  Times the
    sampler's Lipschitz constant: the largest difference of neighbouring taps in the 4 x 4 patch around the cell (zeros outside),
    which also covers a floor that lands in the neighbouring cell.
    Products: the weights 1 - w and w carry an absolute error <= U each, their product, the product with the tap and the three
    additions one rounding each: <= 8 U sum |four taps|."""
    out = []
    for l, c in enumerate(corr):
        n, H, W = c.shape
        cx, cy, px, py = _lk_positions(qx, qy, flow, l, r)
        dx = U * (np.abs(cx)[:, None, None] / 2 ** l + 5 * np.abs(px) + (W - 1) / 2)
        dy = U * (np.abs(cy)[:, None, None] / 2 ** l + 5 * np.abs(py) + (H - 1) / 2)
        x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        o = np.arange(-1, 3)
        P = _taps64(c.astype(np.float64), (y0[..., None, None] + o[:, None]) + 0 * o[None, :], (x0[..., None, None] + o[None, :]) + 0 * o[:, None])
        lx = np.abs(P[..., :, 1:] - P[..., :, :-1]).max(axis=(-1, -2))
        ly = np.abs(P[..., 1:, :] - P[..., :-1, :]).max(axis=(-1, -2))
        rnd = 8 * U * np.abs(P[..., 1:3, 1:3]).sum(axis=(-1, -2))
        out.append((dx * lx + dy * ly + rnd + 1e-37).reshape(n, -1))
    return np.concatenate(out, axis=1)


def lookup_restated(corr, qx, qy, flow, r):
    """corr_lookup_kernel line by line in numpy fp32 (every operation rounded; the device may fuse the last sum's multiply-adds)"""
    out = []
    d = np.arange(-r, r + 1).astype(F32)
    cx, cy = qx.astype(F32) + flow[:, 0], qy.astype(F32) + flow[:, 1]
    for l, c in enumerate(corr):
        n, H, W = c.shape
        div = F32(1 << l)
        px = ((cx / div)[:, None, None] + d[None, :, None] + F32(0) * d[None, None, :]).astype(F32)
        py = ((cy / div)[:, None, None] + d[None, None, :] + F32(0) * d[None, :, None]).astype(F32)
        gx, gy = F32(2) * px / F32(W - 1) - F32(1), F32(2) * py / F32(H - 1) - F32(1)
        ix, iy = (gx + F32(1)) * F32(0.5) * F32(W - 1), (gy + F32(1)) * F32(0.5) * F32(H - 1)
        assert ix.dtype == F32 and gy.dtype == F32
        fx0, fy0 = np.floor(ix), np.floor(iy)
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        wx1, wy1 = ix - fx0, iy - fy0
        wx0, wy0 = F32(1) - wx1, F32(1) - wy1
        at = lambda yy, xx: _taps64(c, yy, xx).astype(F32)
        s = at(y0, x0) * (wx0 * wy0) + at(y0, x0 + 1) * (wx1 * wy0) + at(y0 + 1, x0) * (wx0 * wy1) + at(y0 + 1, x0 + 1) * (wx1 * wy1)
        assert s.dtype == F32
        out.append(s.reshape(n, -1))
    return np.concatenate(out, axis=1)


def lookup_centre_taps(corr, qx, qy, flow, r):
    """[n, levels, 4] bool: which of the four bilinear taps of the window CENTRE of every level lie inside the map"""
    res = []
    for l, c in enumerate(corr):
        n, H, W = c.shape
        _, _, px, py = _lk_positions(qx, qy, flow, l, r)
        x0, y0 = np.floor(px[:, r, r]).astype(np.int64), np.floor(py[:, r, r]).astype(np.int64)
        res.append(np.stack([(y0 + a >= 0) & (y0 + a < H) & (x0 + b >= 0) & (x0 + b < W) for a in (0, 1) for b in (0, 1)], axis=-1))
    return np.stack(res, axis=1)


# ------------------------------------------------------------------------------------------------------------ convex up-sampling
UP_FAMILIES = ("normal", "onehot", "equal", "border")
UP_SHAPES = [(2, 2), (2, 3), (16, 20), (22, 21)]
UP_BORDER_BIAS = 3.0


def up_outside(h, w):
    """[h, w, 9] bool: neighbour k = ky 3 + kx of cell (y, x) lies outside the map"""
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(9), indexing="ij")
    yy, xx = y + k // 3 - 1, x + k % 3 - 1
    return (yy < 0) | (yy >= h) | (xx < 0) | (xx >= w)


def up_inputs(h, w, family, seed, B=2):
    """flow [B, h, w, 2]; mask [B, h, w, 576], channel k 64 + i 8 + j.  Families: unit normal logits; normal times 30 (near one-hot:
    the other eight exponentials underflow); all logits equal; normal plus UP_BORDER_BIAS on the taps that lie outside the map."""
    rng = np.random.default_rng(seed)
    flow = (5.0 * rng.standard_normal((B, h, w, 2))).astype(F32)
    m = rng.standard_normal((B, h, w, 9, 64))
    if family == "onehot":
        m *= 30.0
    elif family == "equal":
        m[:] = 1.25
    elif family == "border":
        m += UP_BORDER_BIAS * up_outside(h, w)[None, ..., None]
    return flow, m.reshape(B, h, w, 576).astype(F32)


def up_ref64(flow, mask, route="torch"):
    """upsample_data (raft.py:183-199) -> float64 [B, 2, 8 h, 8 w].  route 'torch': view, softmax, F.unfold, as the reference writes
    it; route 'explicit': exponentials and a zero-padded neighbourhood by hand."""
    B, h, w, _ = flow.shape
    if route == "torch":
        f, m = _t64(flow).permute(0, 3, 1, 2), _t64(mask).permute(0, 3, 1, 2)
        m = torch.softmax(m.reshape(B, 1, 9, 8, 8, h, w), dim=2)
        uf = F.unfold(8 * f, [3, 3], padding=1).view(B, 2, 9, 1, 1, h, w)
        return torch.sum(m * uf, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 8 * h, 8 * w).numpy()
    p, nb, _ = _up_parts(flow, mask)
    o = (p[..., None] * nb[:, :, :, :, None, :]).sum(axis=3)                       # [B, h, w, 64, 2]
    return o.reshape(B, h, w, 8, 8, 2).transpose(0, 5, 1, 3, 2, 4).reshape(B, 2, 8 * h, 8 * w)


def _up_parts(flow, mask):
    """softmax p [B, h, w, 9, 64], neighbours 8 flow [B, h, w, 9, 2] (zero outside), a = max logit - logit [B, h, w, 9, 64]; float64"""
    B, h, w, _ = flow.shape
    m = mask.astype(np.float64).reshape(B, h, w, 9, 64)
    a = m.max(axis=3, keepdims=True) - m
    e = np.exp(-a)
    p = e / e.sum(axis=3, keepdims=True)
    fp = np.zeros((B, h + 2, w + 2, 2))
    fp[:, 1:-1, 1:-1] = 8.0 * flow.astype(np.float64)
    nb = np.stack([fp[:, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], axis=3)
    return p, nb, a


def up_tol(flow, mask):
    """[B, 2, 8 h, 8 w].  out = sum_k p_k (8 f_k), p_k = e_k / sum_j e_j, e_k = expf(fl(m_k - max)).  Relative error of e_k:
    U |a_k| from the rounded argument a_k = max - m_k plus EXPF_ULPS ulps (2 EXPF_ULPS U) of expf itself; of the denominator: its
    eight additions and the p-weighted mean of the e_j's errors; the division, the product with 8 f_k (8 f is exact) and the nine
    accumulating additions one rounding each.  So |error| <= U sum_k p_k |8 f_k| (|a_k| + A + 4 EXPF_ULPS + 20), A = sum_j p_j |a_j|;
    taps outside the map contribute nothing to the sum but keep their share of the softmax.  Where the largest weight sits on a tap
    outside the map the output is one small term whose error IS the rounded argument's, U |a_k| with a_k in the thirties: the bound is
    attained by fp32 itself, so the tolerance is twice it (fp32 in this order then provably uses at most half)."""
    B, h, w, _ = flow.shape
    p, nb, a = _up_parts(flow, mask)
    A = (p * a).sum(axis=3, keepdims=True)
    t = 2 * U * ((p * (a + A + 4 * EXPF_ULPS + 20))[..., None] * np.abs(nb)[:, :, :, :, None, :]).sum(axis=3) + 1e-30
    return t.reshape(B, h, w, 8, 8, 2).transpose(0, 5, 1, 3, 2, 4).reshape(B, 2, 8 * h, 8 * w)


def up_restated(flow, mask, renormalise_inside=False):
    """convex_upsample_kernel in numpy fp32.  renormalise_inside: the WRONG softmax, over the taps inside the map only."""
    B, h, w, _ = flow.shape
    m = mask.reshape(B, h, w, 9, 64)
    out_k = up_outside(h, w)[None, :, :, :, None]
    mx = m.max(axis=3, keepdims=True)
    e = np.exp((m - mx).astype(np.float64)).astype(F32)          # expf of the fp32 argument, correctly rounded (numpy's own float32 exp
    #                                                              is documented to 2.5 ulp: it would use up the allowance by itself)
    if renormalise_inside:
        e = np.where(out_k, F32(0), e)
    den = np.zeros((B, h, w, 64), F32)
    for k in range(9):
        den = den + e[:, :, :, k]
    fp = np.zeros((B, h + 2, w + 2, 2), F32)
    fp[:, 1:-1, 1:-1] = F32(8) * flow
    o = np.zeros((B, h, w, 64, 2), F32)
    for k in range(9):
        p = e[:, :, :, k] / den
        o = o + p[..., None] * fp[:, k // 3:k // 3 + h, k % 3:k % 3 + w][:, :, :, None, :]      # (a tap outside adds p * 0)
    assert o.dtype == F32
    return o.reshape(B, h, w, 8, 8, 2).transpose(0, 5, 1, 3, 2, 4).reshape(B, 2, 8 * h, 8 * w)


def up_border_pixels(h, w):
    """[8 h, 8 w] bool: output pixels of cells on the map's border"""
    cell = np.zeros((h, w), bool)
    cell[[0, -1], :] = True
    cell[:, [0, -1]] = True
    return np.repeat(np.repeat(cell, 8, axis=0), 8, axis=1)


# ------------------------------------------------------------------------------------------------------------ the movers
# pack_cols: (rows, ldd, c0, lds, Cs); the last one copies 2^24 + 7 * 431 elements
PACK_CASES = [(1, 1, 0, 1, 1), (7, 9, 3, 5, 4), (300, 192, 128, 96, 62), (321, 6, 0, 6, 2)]
PACK_CAP = (38927, 440, 9, 431, 431)                        # 38927 * 431 = 2^24 + 321: the last 321 elements are second trips
SCALE_CASES = [1, 255, 257, 70001]
SCALE_CAP = CAP + 12345
ADD_CASES = [(1, 2), (129, 6), (4097, 3)]                   # (rows, ldu)
# image_absmax: (images, n_per); a launch has min(64, ceil(n_per / 1024)) workgroups per image, so 64 x 1024 is where the loop starts
ABSMAX_CASES = [(1, 1), (3, 1000), (2, 64 * 1024 - 1), (3, 64 * 1024 + 77), (2, 3 * 64 * 1024 + 5)]


def pack_restated(dst, c0, src, Cs):
    out = dst.copy()
    out[:, c0:c0 + Cs] = src[:, :Cs]
    return out


def absmax_inputs(images, n_per, seed):
    """[images, n_per]: image 0 has its single maximum in the last element, image 1 a negative maximum, the others random"""
    x = np.random.default_rng(seed).uniform(-1, 1, (images, n_per)).astype(F32)
    x[0, -1] = F32(3.5)
    if images > 1:
        x[1, n_per // 2] = F32(-7.25)
    return x
