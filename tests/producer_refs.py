"""Host side of the producer pins (tests/test_gpu_producers_f64.py, tests/test_producer_refs_cpu.py): inputs, float64 references,
numpy fp32 restatements of the kernels' arithmetic order, and the tolerances.  No GPU, no library call.

Every tolerance here comes from the precision of the formats or from the reference's OWN fp32 evaluation (torch on the CPU),
never from what a kernel returns.  The restatements exist so that the CPU test can show that fp32 arithmetic in the kernels'
order stays inside those tolerances: what the GPU test then catches is a kernel that computes something else."""
import numpy as np
import torch

F32 = np.float32
U24, U22 = 2.0 ** -24, 2.0 ** -22

# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-6
FAMILIES = ("plain", "offset", "const", "spike", "tiny")
CONST_VALUE = 7.25

# (M, D) of a3r_layernorm; of a3r_layernorm_bf3; D of a3r_layernorm_fh2 at M = LN_FH2_M (register classes 1 / 2 / 3, generic)
LN_F32_CASES = [(1, 4), (3, 36), (80, 100), (80, 1280), (5, 2052), (1, 256), (83, 768), (81, 1024)]
LN_BF3_CASES = [(1, 8), (5, 40), (1, 256), (7, 256), (1, 1024), (9, 768), (80, 1280), (6, 32)]
LN_FH2_M = 83
LN_FH2_D = [32, 64, 480, 512, 544, 768, 1024, 1056, 1280, 1536, 1568, 2048]
LN_FH2_PERSISTENT = (16391, 32)          # 4098 workgroups of 4 rows > the 4096 the launcher caps at when statistics are requested
LN_FH2_UNALIGNED_D = 256


def ln_families(M):
    """Family of every row: the five interleaved (row r -> r % 5) when each gets 16 rows, else plain only."""
    if M < 16 * len(FAMILIES):
        return np.zeros(M, np.int64)
    return np.arange(M) % len(FAMILIES)


def ln_inputs(M, D, seed):
    """x [M, D], w [D], b [D] fp32 and the family index of every row.  Rows are drawn independently (no row repeats, the const
    family apart, which is one row by definition)."""
    rng = np.random.default_rng(seed)
    fam = ln_families(M)
    g = rng.standard_normal((M, D))
    x = np.empty((M, D), np.float64)
    for r in range(M):
        f = FAMILIES[fam[r]]
        if f == "plain":
            x[r] = 0.5 + 3.0 * g[r]
        elif f == "offset":
            x[r] = 1000.0 + g[r]
        elif f == "const":
            x[r] = CONST_VALUE
        elif f == "spike":
            x[r] = g[r]
            x[r, min(3, D - 1)] = 1e4
        else:
            x[r] = 1e-4 * g[r]
    w, b = rng.standard_normal(D), rng.standard_normal(D)
    return x.astype(F32), w.astype(F32), b.astype(F32), fam


def ln_ref64(x, w, b, eps=LN_EPS):
    """float64 nn.LayerNorm of the fp32 inputs."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    return torch.nn.functional.layer_norm(t(x), (x.shape[-1],), t(w), t(b), eps).numpy()


def ln_torch32(x, w, b, eps=LN_EPS):
    """torch's own fp32 CPU layer_norm: the reference's fp32 evaluation, whose error sets the tolerance."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return torch.nn.functional.layer_norm(t(x), (x.shape[-1],), t(w), t(b), eps).numpy()


def ln_tolerances(x, w, b, fam, ref=None):
    """Per family present in the call: 4 max(e32, 2^-22 max|ref|), e32 = the largest error of torch's fp32 CPU layer_norm over that
    family's rows against float64.  Returns ({family index: tol}, ref)."""
    ref = ln_ref64(x, w, b) if ref is None else ref
    t32 = ln_torch32(x, w, b).astype(np.float64)
    tol = {}
    for f in np.unique(fam):
        rows = fam == f
        e32 = float(np.abs(t32[rows] - ref[rows]).max())
        tol[int(f)] = 4.0 * max(e32, U22 * float(np.abs(ref[rows]).max()))
    return tol, ref


def ln_family_errors(got, ref, fam):
    """{family index: max |got - ref| over its rows}"""
    got = np.asarray(got, np.float64)
    return {int(f): float(np.abs(got[fam == f] - ref[fam == f]).max()) for f in np.unique(fam)}


def _tree64(s):
    """wave_sum (csrc/common.h): a butterfly over lane ^ 1, 2, (4, 8 by the row mirrors), 16, 32 -- a binary tree over the 64 lanes"""
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def _fma32(a, b, c):
    """fmaf of fp32 operands: the product is exact in float64, one rounding of the sum to fp32 (up to a double rounding)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def ln_restated(x, w, b, order, eps=LN_EPS):
    """The kernels' LayerNorm arithmetic in numpy fp32.  order: 'f4' -- a lane sums whole float4 (lane + 64 i), layernorm_kernel and
    layernorm_pair_kernel; 'f8' -- a lane sums two adjacent float4 per step, layernorm_fh2_kernel; 'strided' -- a lane sums
    elements lane + 64 i, the generic kernels.  Then the 64-lane tree, the mean, the centred squares in the same order, fma with
    w and b.  (For D that the launcher gives to another kernel the order is still a valid fp32 order of the same sums.)"""
    x = np.ascontiguousarray(x, F32)
    M, D = x.shape
    per = dict(f4=4, f8=8, strided=1)[order]
    assert D % per == 0
    steps = -(-D // (64 * per))
    pad = steps * 64 * per

    def lanes(v):                                       # [M, D] -> [M, steps, 64, per] with zeros past the row
        p = np.zeros((M, pad), F32)
        p[:, :D] = v
        return p.reshape(M, steps, 64, per)

    def lane_sums(v4, squares):
        if squares:
            v4 = v4 * v4
        s = np.zeros((M, 64), F32)
        for i in range(steps):
            e = v4[:, i]
            if per == 1:
                s = s + e[..., 0]
            else:
                q0 = ((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]
                if per == 4:
                    s = s + q0
                else:
                    q1 = ((e[..., 4] + e[..., 5]) + e[..., 6]) + e[..., 7]
                    s = (s + q0) + q1 if squares else s + (q0 + q1)
        return s
    mean = _tree64(lane_sums(lanes(x), False)) / F32(D)
    c = x - mean[:, None]
    var = _tree64(lane_sums(lanes(c), True)) / F32(D)
    rstd = F32(1.0) / np.sqrt(var + F32(eps))
    return _fma32(c * rstd[:, None], w[None, :].astype(F32), b[None, :].astype(F32))


def fh2_resolution(v, scale):
    """What two fp16 planes of scale * v lose (csrc/fh2.h): 2^-22 relative, 2^-25 / scale absolute where the second plane is
    subnormal; with the factor 2 that tests/test_gpu_fh2_range.py allows.  v: numpy array or torch tensor."""
    return 2.0 ** -21 * abs(v) + 2.0 ** -24 / min(scale, 1.0)


# ------------------------------------------------------------------------------------------------------------ bilinear 2x
# the SHAPES of tests/test_gpu_up2x_forms.py are added by the GPU test; these are the further ones (B, H, W, C, crop)
UP_EXTRA = [
    (1, 33, 17, 8, (65, 34)),
    (1, 300, 3, 4, None),
    (1, 2, 1025, 4, (3, 2049)),
    (4100, 8, 3, 4, None),           # 65600 output rows: the first form's y loop repeats
    (7300, 8, 3, 4, None),           # 65700 block rows: the second form's y loop repeats
]
UP_BF3 = [(2, 7, 9, 64, (13, 18)), (1, 1, 5, 8, None), (1, 4, 1, 16, None), (4100, 8, 3, 8, None)]


def up_input(B, H, W, C, seed):
    return (3.0 * np.random.default_rng(seed).standard_normal((B, H, W, C))).astype(F32)


def _up_axis64(n):
    o = np.arange(2 * n, dtype=np.float64)
    src = o * ((n - 1) / (2 * n - 1)) if n > 1 else np.zeros_like(o)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def up_formula64(x, crop=None):
    """The align_corners=True bilinear 2x written out in float64 (channels last)."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    y0, y1, ly = _up_axis64(H)
    x0, x1, lx = _up_axis64(W)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    out = top * (1 - ly) + bot * ly
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    return out[:, :Hc, :Wc]


def up_ref64(x, crop=None):
    """float64 F.interpolate(scale_factor=2, bilinear, align_corners=True), then the crop; for H = 1 or W = 1 the written-out formula."""
    B, H, W, C = x.shape
    if H == 1 or W == 1:
        return up_formula64(x, crop)
    t = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    return y[:, :Hc, :Wc]


def up_tolerance(x):
    """Per batch item [B, 1, 1, 1]: (2 (H + W) + 8) 2^-24 max|x_b|.  The kernel follows ATen in computing the source coordinate in
    fp32: the rounding of s = (n - 1) / (2 n - 1) moves it by at most 2^-25 n per axis, a value by at most that times
    2 max|x|; four more roundings add 4 x 2^-24."""
    B, H, W, C = x.shape
    return ((2 * (H + W) + 8) * U24 * np.abs(x.astype(np.float64)).reshape(B, -1).max(1)).reshape(B, 1, 1, 1)


def _up_axis32(n):
    """up_scale / up_axis of csrc/elementwise.hip in fp32"""
    s = F32(n - 1) / F32(2 * n - 1) if 2 * n > 1 and n > 1 else F32(0)
    fo = np.arange(2 * n).astype(F32)
    i0 = np.minimum((s * fo).astype(np.int64), n - 1)
    i1 = np.where(i0 < n - 1, i0 + 1, i0)
    l1 = _fma32(np.full_like(fo, s), fo, -i0.astype(F32))
    return i0, i1, F32(1) - l1, l1


def up_restated(x, crop=None):
    """up_axis / bilerp4 in numpy fp32, operation by operation."""
    x = np.ascontiguousarray(x, F32)
    B, H, W, C = x.shape
    y0, y1, ly0, ly1 = _up_axis32(H)
    x0, x1, lx0, lx1 = _up_axis32(W)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    r0, r1 = x[:, y0], x[:, y1]
    t0 = _fma32(r0[:, :, x1], lx1, r0[:, :, x0] * lx0)
    t1 = _fma32(r1[:, :, x1], lx1, r1[:, :, x0] * lx0)
    out = _fma32(t1, ly1, t0 * ly0)
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    return out[:, :Hc, :Wc]


# ------------------------------------------------------------------------------------------------------------ head final
# (P, C): generic kernel with 2, 9, 33 and 64 float4 per pixel (the j += 32 loop from C = 132); its second trip past 131072
# pixels; the C = 128 kernel with one partial step and with a second trip past 262144 pixels whose last step is partial
HEAD_CASES = [(1, 8), (7, 36), (9, 132), (969, 256), (131085, 8), (262157, 128), (31, 128)]
HEAD_SIGMA = 0.8          # standard deviation of the four conv outputs: keeps d and |f3| below 6 (asserted)


def head_inputs(P, C, seed):
    """x [P, C], w [4, C], bias [4] fp32 (torch CPU generator)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(P, C, generator=g)
    w = torch.randn(4, C, generator=g) * (HEAD_SIGMA / C ** 0.5)
    bias = torch.randn(4, generator=g) * 0.1
    return x, w, bias


def head_post(f):
    """postprocess (xyz / d.clip(1e-8) * expm1(d), 1 + exp(f3)) in the dtype of f [P, 4]; also returns d"""
    d = f[:, :3].norm(dim=-1, keepdim=True)
    return f[:, :3] / d.clip(min=1e-8) * torch.expm1(d), 1 + f[:, 3].exp(), d


def head_refs(x, w, bias):
    """-> (pts64, conf64, tol_pts, tol_conf, dmax, f3max): the float64 reference and 4 max(e32, 2^-22 max|ref|) with e32 the error of
    the same steps in torch fp32 on the CPU."""
    f64 = torch.nn.functional.linear(x.double(), w.double(), bias.double())
    p64, c64, d = head_post(f64)
    p32, c32, _ = head_post(torch.nn.functional.linear(x, w, bias))
    tol = lambda a32, a64: 4.0 * max(float((a32.double() - a64).abs().max()), U22 * float(a64.abs().max()))
    return p64, c64, tol(p32, p64), tol(c32, c64), float(d.max()), float(f64[:, 3].abs().max())


def head_restated(x, w, bias):
    """The head kernels' order in numpy fp32: per pixel 32 lanes that each sum the dot products of float4 j = lane, lane + 32, ...
    (C = 128: 8 lanes of 16 consecutive channels), a butterfly over the lanes, the bias, the postprocess in fp32."""
    x, w, bias = x.numpy().astype(F32), w.numpy().astype(F32), bias.numpy().astype(F32)
    P, C = x.shape
    f = np.empty((P, 4), F32)
    for o in range(4):
        prod = x * w[o][None, :]
        if C == 128:
            part = prod.reshape(P, 8, 16)
            lanes = np.zeros((P, 8), F32)
            for k in range(16):
                lanes = lanes + part[:, :, k]
        else:
            nvec = C // 4
            steps = -(-nvec // 32)
            padded = np.zeros((P, steps * 32 * 4), F32)
            padded[:, :C] = prod
            part = padded.reshape(P, steps, 32, 4)
            lanes = np.zeros((P, 32), F32)
            for i in range(steps):
                e = part[:, i]
                lanes = lanes + (((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3])
        f[:, o] = _tree64(lanes) + bias[o]
    d = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2])
    em = np.expm1(d)
    pts = f[:, :3] / np.maximum(d, F32(1e-8))[:, None] * em[:, None]
    return pts, F32(1) + np.exp(f[:, 3])


# ------------------------------------------------------------------------------------------------------------ RoPE-2D
ROPE_BASE = 100.0
ROPE_CASES = [(1, 1, 1, 4, 3), (2, 35, 3, 64, 255), (1, 50, 2, 128, 2000), (4, 4100, 16, 128, 63)]     # (B, N, H, D, pmax)


def rope_inputs(B, N, H, D, pmax, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    tok = torch.randn(B, N, H, D, generator=g)
    pos = torch.randint(0, pmax + 1, (B, N, 2), generator=g, dtype=torch.int64)
    pos.view(-1)[-1] = pmax                                   # the largest position is present
    return tok, pos


def rope_ref64(tok, pos, fwd, base=ROPE_BASE):
    """float64 rotation by fwd p / base^(q / Q), Q = D / 4: half h of a token (channels 2 Q h ... 2 Q h + 2 Q) takes p = pos[..., h]
    and rotates its pairs (q, q + Q).  tok [B, N, H, D] of any float dtype on any device; returns float64."""
    B, N, H, D = tok.shape
    Q = D // 4
    t = tok.double().reshape(B, N, H, 2, 2, Q)
    q = torch.arange(Q, dtype=torch.float64, device=tok.device)
    ang = fwd * pos.double()[:, :, None, :, None] / (base ** (q / Q))          # [B, N, 1, 2, Q]
    c, s = torch.cos(ang), torch.sin(ang)
    u, v = t[..., 0, :], t[..., 1, :]
    return torch.stack([u * c - v * s, v * c + u * s], dim=-2).reshape(B, N, H, D)


def rope_tolerance(tok, pmax):
    """Per element (both of a pair): (4 pmax + 8) 2^-24 hypot(u, v) -- the fp32 angle carries the error."""
    B, N, H, D = tok.shape
    t = tok.double().reshape(B, N, H, 2, 2, D // 4)
    h = torch.hypot(t[..., 0, :], t[..., 1, :])
    return (4 * pmax + 8) * U24 * torch.stack([h, h], dim=-2).reshape(B, N, H, D)


def rope_restated(tok, pos, fwd, base=ROPE_BASE):
    """rope2d_kernel in numpy fp32 (powf, cosf, sinf as numpy's fp32 functions)."""
    tok = tok.numpy().astype(F32)
    B, N, H, D = tok.shape
    Q = D // 4
    t = tok.reshape(B, N, H, 2, 2, Q)
    q = np.arange(Q).astype(F32)
    p = pos.numpy().astype(F32)[:, :, None, :, None]
    ang = (F32(fwd) * p / np.power(F32(base), q / F32(Q))).astype(F32)
    c, s = np.cos(ang), np.sin(ang)
    u, v = t[..., 0, :], t[..., 1, :]
    return np.stack([u * c - v * s, v * c + u * s], axis=-2).reshape(B, N, H, D), ang


# ------------------------------------------------------------------------------------------------------------ grid-stride copies
PATCHIFY_SHAPE = (6, 3, 1024, 1024)              # 18.9 M elements > 65536 x 256
GATHER_ADD_SHAPE = (9, 2048, 3648, 3, 2)         # S, N, C, Ua, Ub: 16.81 M float4 > 65536 x 256
GATHER_MAP_A = [2, 0, 1, 1, 2, 0, 0, 2, 1]
GATHER_MAP_B = [0, 1, 1, 0, 0, 0, 1, 1, 1]
