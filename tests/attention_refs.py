"""Host side of the attention pins (tests/test_gpu_attention_f64.py, tests/test_attention_refs_cpu.py): input families built from a
designed score profile, the float64 truth with its per-row scales, the tolerance, and numpy fp32 restatements of the kernels'
arithmetic order.  No GPU, no library call.

Nothing in a tolerance comes from a kernel: it is made of the error of torch's own fp32 CPU evaluation of the reference formula
(softmax(q k^T / 8) v, croco/models/blocks.py:105-109), of the precision of the operand format (2^-22, csrc/fh2.h) and of the
format's absolute floor (2^-25 / scale).  The restatements exist so that the CPU test can show that fp32 arithmetic in the kernels'
order stays inside the tolerance WITHOUT its factor 4: what the GPU test then catches is a kernel that computes something else."""
import functools

import numpy as np
import torch

F32, F16 = np.float32, np.float16
U22, U25, U12 = 2.0 ** -22, 2.0 ** -25, 2.0 ** -12
HD = 64
LOG2E_F32 = F32(1.4426950408889634)
PSHIFT = F32(10.0)                       # ATTN_PSHIFT of csrc/attention_tile.h: P is carried as 2^10 p

FAMILIES = ("plain", "sharp", "ties", "voff", "ramp", "peak0", "peakmid", "peaklast", "high", "low")

# (Nq, Nk) of the GPU file: the smallest shapes on each side of a 32-key block, a 64-key tile and a 32-query / 128-query block;
# (257, 197): three query blocks, four key tiles (both K buffers reused); (40, 321): six tiles, the last one holding one key
SHAPES = [(1, 1), (1, 33), (31, 31), (32, 32), (33, 33), (33, 63), (64, 64), (65, 65), (33, 97), (127, 129), (128, 128), (129, 130),
          (257, 197), (40, 321)]
SINGLE_PASS_SHAPES = [(33, 33), (65, 65), (129, 130), (257, 197)]
LAYOUT_SHAPES = [(33, 97), (129, 130)]
GROUP_SHAPE = (129, 130)
GROUP_COUNTS = [(1, 1), (7, 1), (2, 4), (3, 3), (17, 1)]            # (B, H): B H = 1, 7, 8, 9, 17 groups on 8 slots
LAUNCH_B, LAUNCH_H = 2, 5                                           # ten groups: one per family


def case_seed(family, Nq, Nk):
    return FAMILIES.index(family) * 1000003 + Nq * 1009 + Nk


def peak_index(family, Nk):
    return {"peak0": 0, "peakmid": Nk // 2, "peaklast": Nk - 1}[family]


def attn_inputs(family, Nq, Nk, seed):
    """fp32 q [Nq, 64], k [Nk, 64], v [Nk, 64] of one head.  The structured families follow a designed score profile: with u a
    random unit vector, q_i = 8 beta_i u + noise and k_j = a_j u + noise give score_ij = q_i k_j / 8 ~ beta_i a_j."""
    rng = np.random.default_rng(seed)
    gq, gk, v = rng.standard_normal((Nq, HD)), rng.standard_normal((Nk, HD)), rng.standard_normal((Nk, HD))
    u = rng.standard_normal(HD)
    u /= np.linalg.norm(u)
    beta = rng.uniform(0.75, 1.25, Nq)
    j = np.arange(Nk, dtype=np.float64)
    if family == "plain":
        q, k = gq, gk
    elif family == "sharp":
        q, k = 4.0 * gq, 3.0 * gk
    elif family == "ties":
        q, k = gq, np.repeat(gk[:1], Nk, axis=0)
    elif family == "voff":
        q, k, v = gq, gk, v + 100.0
    elif family == "ramp":
        # the key noise is kept out of the u direction and small: the profile rises by 0.05 beta per key, and a last block of a
        # single key (Nk = 65, 129, 321) must still carry the maximum
        gk = gk - np.outer(gk @ u, u)
        q, k = 8.0 * beta[:, None] * u + 0.1 * gq, np.outer(0.05 * j, u) + 0.02 * gk
    elif family in ("peak0", "peakmid", "peaklast"):
        a = np.zeros(Nk)
        a[peak_index(family, Nk)] = np.log(max(Nk - 1, 1))
        q, k = 8.0 * beta[:, None] * u + 0.1 * gq, np.outer(a, u) + 0.1 * gk
    elif family in ("high", "low"):
        a = 70.0 if family == "high" else -70.0
        q, k = 8.0 * u + gq, a * u + gk
    else:
        raise ValueError(family)
    return q.astype(F32), k.astype(F32), v.astype(F32)


# ------------------------------------------------------------------------------------------------------------ truth and tolerance
def scores64(q, k):
    return q.astype(np.float64) @ k.astype(np.float64).T / 8.0


def softmax64(s):
    e = np.exp(s - s.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def attn_truth(q, k, v):
    """-> (out [Nq, 64], R [Nq], A [Nq], p [Nq, Nk]) in float64: softmax(q k^T / 8) v of the fp32 inputs; R_i = max_d sum_k p_ik |v_kd|,
    the row's output scale; A_i = max_k sum_d |q_id k_kd| / 8, the condition number of the row's scores."""
    p = softmax64(scores64(q, k))
    v64 = v.astype(np.float64)
    R = (p @ np.abs(v64)).max(1)
    A = (np.abs(q.astype(np.float64)) @ np.abs(k.astype(np.float64)).T).max(1) / 8.0
    return p @ v64, R, A, p


def attn_torch32(q, k, v):
    """torch's own fp32 CPU evaluation of the reference formula (blocks.py:105-109)"""
    t = lambda a: torch.from_numpy(np.array(a, F32))
    attn = (t(q) @ t(k).transpose(-2, -1)) * (HD ** -0.5)
    return (attn.softmax(dim=-1) @ t(v)).numpy()


def first_planes(x, scale):
    """rn_f16(scale x) / scale: what the single-pass mode multiplies"""
    return ((x.astype(F32) * F32(scale)).astype(F16).astype(np.float64) / scale)


class Case:
    """One (family, shape) head: inputs, truth and the pieces of the tolerance."""

    def __init__(self, q, k, v, single_pass_scales=None):
        self.q, self.k, self.v = q, k, v
        if single_pass_scales is None:
            tq, tk, tv = q, k, v
        else:                                               # truth of the single-pass mode: the first planes, in float64
            qs, ks, vs = single_pass_scales
            tq, tk, tv = first_planes(q, qs), first_planes(k, ks), first_planes(v, vs)
        self.ref, self.R, self.A, self.p = attn_truth(tq, tk, tv)
        t32 = attn_torch32(tq, tk, tv).astype(np.float64)
        self.e32 = float((np.abs(t32 - self.ref).max(1) / self.R).max())
        self.single = single_pass_scales is not None

    def bound(self, v_scale=None, out_scale=None):
        """[Nq]: max(e32, 2^-22 (1 + A_i)) R_i + 2^-25 (1 / v_scale + 1 / out_scale) -- the tolerance without its factor 4.  The
        floor term belongs to the fh2 form (scales given); it is zero for the fp32 and bf3 kernels."""
        floor = 0.0 if v_scale is None else U25 * (1.0 / v_scale + 1.0 / out_scale)
        return np.maximum(self.e32, U22 * (1.0 + self.A)) * self.R + floor

    def tol(self, v_scale=None, out_scale=None):
        """[Nq]: tol_i = 4 bound_i (+ 2^-12 R_i in the single-pass mode: every P entry is rounded once to fp16 while l sums the
        unrounded values)."""
        t = 4.0 * self.bound(v_scale, out_scale)
        return t + U12 * self.R if self.single else t

    def row_errors(self, got):
        return np.abs(np.asarray(got, np.float64) - self.ref).max(1)


@functools.lru_cache(maxsize=None)
def attn_case(family, Nq, Nk, mul=(1.0, 1.0, 1.0), single_pass_scales=None):
    """The cached case of (family, shape); mul: powers of two on q, k, v (the scaled launch), exact in fp32."""
    q, k, v = attn_inputs(family, Nq, Nk, case_seed(family, Nq, Nk))
    q, k, v = q * F32(mul[0]), k * F32(mul[1]), v * F32(mul[2])
    for a in (q, k, v):
        a.setflags(write=False)
    return Case(q, k, v, single_pass_scales)


def check_family_conditions(family, case):
    """The conditions that make a family reach what it is there for, asserted in float64."""
    Nq, Nk = case.q.shape[0], case.k.shape[0]
    s, p = scores64(case.q, case.k), case.p
    if family == "ramp" and Nk >= 65:
        nb = -(-Nk // 32)
        bmax = np.stack([s[:, 32 * b:32 * b + 32].max(1) for b in range(nb)], 1)
        assert (np.diff(bmax, axis=1) > 0).all(), ("ramp: the running maximum does not rise at every block", Nq, Nk)
        outside = p[:, :32 * (nb - 1)].sum(1)
        assert outside.min() >= 0.10, ("ramp: mass outside the last block", Nq, Nk, float(outside.min()))
    if family.startswith("peak") and Nk >= 33:
        pk = peak_index(family, Nk)
        assert (s.argmax(1) == pk).all(), (family, Nq, Nk)
        assert 0.15 <= p[:, pk].min() and p[:, pk].max() <= 0.85, (family, Nq, Nk, float(p[:, pk].min()), float(p[:, pk].max()))
    if family in ("high", "low"):
        assert np.abs(s).min() >= 30.0, (family, Nq, Nk, float(np.abs(s).min()))
        assert (s > 0).all() if family == "high" else (s < 0).all()
    if family == "ties":
        assert np.abs(p - 1.0 / Nk).max() <= 1e-12, (Nq, Nk)


# ------------------------------------------------------------------------------------------------------------ launch layout
def launch_groups(shape_index, groups=LAUNCH_B * LAUNCH_H):
    """family of every (batch, head) group of a launch: family f sits in group (f + shape_index) % 10; launches with another group
    count cycle through the families from the same start"""
    fams = [None] * groups
    for g in range(groups):
        fams[g] = FAMILIES[(g - shape_index) % len(FAMILIES)]
    return fams


def assemble(fams, B, H, Nq, Nk, mul=(1.0, 1.0, 1.0), single_pass_scales=None):
    """-> q [B Nq, H 64], k, v [B Nk, H 64] fp32 and the Case of every group (group g = b H + h)"""
    q = np.empty((B * Nq, H * HD), F32)
    k, v = np.empty((B * Nk, H * HD), F32), np.empty((B * Nk, H * HD), F32)
    cases = []
    for g, fam in enumerate(fams):
        b, h = divmod(g, H)
        c = attn_case(fam, Nq, Nk, mul, single_pass_scales)
        q[b * Nq:(b + 1) * Nq, h * HD:(h + 1) * HD] = c.q
        k[b * Nk:(b + 1) * Nk, h * HD:(h + 1) * HD] = c.k
        v[b * Nk:(b + 1) * Nk, h * HD:(h + 1) * HD] = c.v
        cases.append(c)
    return q, k, v, cases


def group_block(out, g, H, Nq):
    """rows and columns of group g in an output [B Nq, >= H 64]"""
    b, h = divmod(g, H)
    return out[b * Nq:(b + 1) * Nq, h * HD:(h + 1) * HD]


# ------------------------------------------------------------------------------------------------------------ restatements
def _f32(a):
    return np.asarray(a, np.float64).astype(F32)


def _split_fh2(x, scale):
    """fh2.h: h0 = rn_f16(s x), h1 = rn_f16(s x - h0), as fp32 arrays"""
    xs = x.astype(F32) * F32(scale)
    h0 = xs.astype(F16).astype(F32)
    return h0, (xs - h0).astype(F16).astype(F32)


def _mma(acc, a, b):
    """one matrix instruction: exact products, one rounding of acc + a b^T to fp32"""
    return (acc.astype(np.float64) + a.astype(np.float64) @ b.astype(np.float64).T).astype(F32)


def _lane_keys(block, half):
    """the keys of a block that lane half `half` of a query holds, in accumulator order (kt, e)"""
    return [kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * half for kt in range(block // 32) for e in range(16)]


FAULTS = ("no_rescale", "mask_over", "mask_under", "no_cross", "no_p1")


def _online(q, k, v, fh2, scales, passes, block, fault):
    assert fault is None or fault in FAULTS
    Nq, Nk = q.shape[0], k.shape[0]
    qs, ks, vs, os_ = scales
    if fh2:
        q0, q1 = _split_fh2(q, qs)
        k0, k1 = _split_fh2(k, ks)
        v0, v1 = _split_fh2(v, vs)
        c = F32(F32(0.125) * LOG2E_F32 / (F32(qs) * F32(ks)))           # scale_log2e of the launcher
    else:
        q0, k0, v0 = q.astype(F32) * F32(0.125), k.astype(F32), v.astype(F32)
        c = LOG2E_F32
    cross = fh2 and passes == 3 and fault != "no_cross"
    two_p = fh2 and passes == 3 and fault != "no_p1"
    valid = Nk + 1 if fault == "mask_over" else Nk - 1 if fault == "mask_under" else Nk      # keys below `valid` pass the mask
    ntiles = -(-Nk // 64)
    oacc = np.zeros((Nq, HD), F32)
    m_run = np.full(Nq, -np.inf, F32)
    l_run = np.zeros((Nq, 2), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for blk in range(ntiles * 64 // block):
            key = np.minimum(np.arange(blk * block, (blk + 1) * block), Nk - 1)    # rows past Nk: copies of the last key
            live = np.arange(blk * block, (blk + 1) * block) < valid
            # ---- S = Q K^T
            s = np.zeros((Nq, block), F32)
            if fh2:
                for st in range(4):
                    d = slice(16 * st, 16 * st + 16)
                    if cross:
                        s = _mma(s, q0[:, d], k1[key, d])
                        s = _mma(s, q1[:, d], k0[key, d])
                    s = _mma(s, q0[:, d], k0[key, d])
            else:
                for kb in range(8):
                    for tt in range(4):
                        d = [8 * kb + tt, 8 * kb + 4 + tt]
                        s = _mma(s, q0[:, d], k0[key][:, d])
            s[:, ~live] = -np.inf
            # ---- online softmax
            m_new = np.maximum(m_run, s.max(1))
            alpha = np.exp2(((m_run - m_new) * c).astype(F32)).astype(F32)
            m_run = m_new
            if fh2:
                off = _f32(-m_new.astype(np.float64) * np.float64(c) + np.float64(PSHIFT))
                p = np.exp2(_f32(s.astype(np.float64) * np.float64(c) + off[:, None].astype(np.float64))).astype(F32)
            else:
                p = np.exp2(((s - m_new[:, None]) * c).astype(F32)).astype(F32)
            for half in range(2):
                lsum = np.zeros(Nq, F32)
                for kk in _lane_keys(block, half):
                    lsum = lsum + p[:, kk]
                l_run[:, half] = l_run[:, half] * alpha + lsum
            if fault != "no_rescale":
                oacc = oacc * alpha[:, None]
            # ---- O += P V
            if fh2:
                p0 = p.astype(F16).astype(F32)
                p1 = (p - p0).astype(F16).astype(F32)
                for s2 in range(block // 16):
                    kk = slice(16 * s2, 16 * s2 + 16)
                    if passes == 3:
                        oacc = _mma(oacc, p0[:, kk], v1[key[kk]].T)
                        if two_p:
                            oacc = _mma(oacc, p1[:, kk], v0[key[kk]].T)
                    oacc = _mma(oacc, p0[:, kk], v0[key[kk]].T)
            else:
                vz = v0[key]
                for kt in range(block // 32):
                    for e in range(16):
                        kk = [kt * 32 + (e & 3) + 8 * (e >> 2), kt * 32 + (e & 3) + 8 * (e >> 2) + 4]
                        oacc = _mma(oacc, p[:, kk], vz[kk].T)
        l_tot = l_run[:, 0] + l_run[:, 1]
        inv_l = (F32(os_) / F32(vs) if fh2 else F32(1)) / l_tot
        out = oacc * inv_l[:, None]
    if not fh2:
        return out
    h0 = out.astype(F16).astype(F32)
    h1 = (out - h0).astype(F16).astype(F32)
    return (h0.astype(np.float64) + h1.astype(np.float64)) / os_


def attn_restate_fh2(q, k, v, scales=(1.0, 1.0, 1.0, 1.0), passes=3, fault=None):
    """attn_fh2_v2_kernel (and attn_fh2_kernel: the same products in the same order) in numpy fp32; scales = (q, k, v, out).
    Operands split as fh2.h says; scores h0 g1 + h1 g0, then h0 g0, per 16-deep step; online softmax in 32-key blocks with
    off = fma(-m, c, 10) and alpha from (m_run - m_new) c; l summed per lane half before P is split into two fp16 planes of
    1024 p; keys past Nk are copies of the last key, masked to -inf; the output stored as two planes of out_scale o.  Returns
    the float64 value of the stored planes.  passes = 1: first planes only, P rounded to one fp16.
    fault: one of FAULTS -- the same order, wrong in one place (tests/test_attention_refs_cpu.py)."""
    return _online(q, k, v, True, scales, passes, 32, fault)


def attn_restate_f32(q, k, v, block=32, fault=None):
    """The same order in plain fp32: q pre-scaled by 1/8, p = exp2((s - m) log2 e), every product one fp32 matrix step.  block = 64
    is attn_kernel's tile (one softmax step per 64 keys), block = 32 attn_bf3_kernel's (its three planes sum to the fp32 operand
    exactly, so six products are the fp32 product in another order)."""
    return _online(q, k, v, False, (1.0, 1.0, 1.0, 1.0), 3, block, fault)
