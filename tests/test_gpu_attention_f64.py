"""GPU: the three attention kernels (csrc/attention.hip, attention_bf3.hip, attention_fh2.hip: both forms and the single-pass mode)
against float64, on ten score families and at the smallest shapes on each side of every block and tile edge.

The existing attention tests draw q, k, v from N(0, 1): a nearly flat softmax whose running maximum settles in the first tile.  Here
every launch holds ten (batch, head) groups (B = 2, H = 5: more than the eight workgroup slots of the group mapping), one per family
of tests/attention_refs.py -- sharp, exactly flat, large V, a maximum that moves in every 32-key block, a peak key first / in the
middle / last that holds half the mass, scores near +70 and near -70 -- and every group is judged row by row against

    tol_i = 4 max(e32, 2^-22 (1 + A_i)) R_i + 4 2^-25 (1 / v_scale + 1 / out_scale)        (last term: the fh2 form only)

R_i = max_d sum_k p_ik |v_kd|, A_i = max_k sum_d |q_id k_kd| / 8, e32 = the R-normalised error of torch's own fp32 CPU evaluation
of the reference formula over the rows of that group.  Nothing in it comes from a kernel; tests/test_attention_refs_cpu.py shows
that fp32 arithmetic in the kernels' order meets it without the factor 4 and that a mask off by one, a skipped rescale, dropped
cross terms or a dropped second plane of P exceed it.  The single-pass mode is judged against float64 attention on the first fp16
planes with 2^-12 R_i added (P rounded once to fp16).

What reaches what (csrc/attention_fh2.hip):
  key mask beside clamped rows            peaklast (the last valid key decides half the result), ties, low (fp32 kernel: a phantom
                                          zero row would take the whole softmax), at Nk = 1, 31, 33, 63, 65, 97, 129, 130, 197, 321
  empty second block (Nk % 64 <= 32)      Nk = 1, 31, 32, 65, 97, 129, 130, 197 (5), 321 (1)
  rescale skipped under ballot(alpha!=1)  peak0 (never moves) beside ramp (moves in every block) in ONE launch; peakmid, peaklast
  off rounded apart from alpha            high, low
  P in two planes of 1024 p, l, halves    every family; ties pins l (exactly flat), voff the cancellation-free sum
  group mapping, surplus workgroups       ten groups per launch; test_group_counts: 1, 7, 8, 9, 17 groups with two query blocks
  output statistic                        every fh2 launch; test_statistic_ignores_rows_past_nq

Measured on an MI355X (worst error / tol_i over the shapes; every figure goes through conftest.record_margin, the table per family
is in DESIGN.md section 2):
  a3r_attention (fp32)          0.22 (peak0, 40 x 321)        a3r_attention_bf3             0.15 (high, 128 x 128)
  a3r_attention_fh2, both forms 0.13 (peaklast, 33 x 33)      scales 2^6 / 2^10             0.19 (voff, 129 x 130)
  single pass, own bound        0.67 (sharp, 65 x 65)         scaled inputs at scale 1      0.15, and 41 without the floor term"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_refs as R
from conftest import record_margin
from align3r_amd import _lib

pytestmark = pytest.mark.gpu

B0, H0 = R.LAUNCH_B, R.LAUNCH_H
ONES = (1.0, 1.0, 1.0, 1.0)
SCALED_MUL, SCALED = (2.0 ** -6, 2.0 ** -6, 2.0 ** -10), (2.0 ** 6, 2.0 ** 6, 2.0 ** 10, 2.0 ** 10)
GUARD = 16


@pytest.fixture(scope="module")
def ops():
    from align3r_amd import ops as o
    assert o.bf3_set_products(6) == 6 and o.fh2_set_passes(3) == 3          # the default modes: six products, three passes
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def judge(name, out, cases, fams, H, Nq, **scales):
    """out [B Nq, >= H 64] (float64-convertible, host): every group row by row against its own tol_i; logs and asserts the worst
    error / tol_i per family"""
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), name
    worst = {}
    for g, (fam, c) in enumerate(zip(fams, cases)):
        ratio = float((c.row_errors(R.group_block(out, g, H, Nq)) / c.tol(**scales)).max())
        worst[fam] = max(worst.get(fam, 0.0), ratio)
    record_margin(name, **worst)
    bad = {f: r for f, r in worst.items() if not r <= 1.0}
    assert not bad, (name, bad)
    return worst


# ------------------------------------------------------------------------------------------------------------ launches
def run_f32(q, k, v, B, H, Nq, Nk):
    D = H * 64
    o = torch.full((B * Nq, D), float("nan"), device="cuda")
    _lib.check(_lib.load().a3r_attention(p(q), D, p(k), D, p(v), D, p(o), D, B, H, Nq, Nk, _lib.stream_ptr()), "attention")
    return o.cpu().numpy()


def bf3_value(o3):
    return o3.planes().double().sum(0).cpu().numpy()


def check_statistic(ops, o2, word):
    """the range word of an fh2 launch: set, and max |h0 + h1| of the stored planes within 2^-22 relative (fh2.h: the two planes
    carry 22 bits of a stored value >= 2^-3; below that the second plane is subnormal and the format's bound is 2^-25 absolute)"""
    got = ops.absmax_value(word)
    pl = o2.planes().double()
    stored = float((pl[0] + pl[1]).abs().max())
    assert got > 0 and int(word.item()) != 0
    assert abs(got - stored) <= (R.U22 * stored if stored >= 0.125 else R.U25), (got, stored)
    return got


def run_fh2(ops, q2, k2, v2, B, H, Nq, Nk, out_scale=1.0, **cols):
    word = ops.absmax_word("cuda")
    o2 = ops.attention_fh2(q2, k2, v2, B, H, Nq, Nk, out_scale=out_scale, out_absmax=word, **cols)
    check_statistic(ops, o2, word)
    return o2


class form:
    """with form(n): a3r_attention_fh2 launches kernel form n; the previous form is restored"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.prev = _lib.load().a3r_attention_fh2_set_form(self.n)
        assert self.prev in (1, 2)

    def __exit__(self, *exc):
        _lib.load().a3r_attention_fh2_set_form(self.prev)


def launch_case(si, B=B0, H=H0, mul=(1.0, 1.0, 1.0), single=None):
    Nq, Nk = R.SHAPES[si]
    fams = R.launch_groups(si, B * H)
    q, k, v, cases = R.assemble(fams, B, H, Nq, Nk, mul, single)
    return fams, cases, dev(q), dev(k), dev(v)


# ------------------------------------------------------------------------------------------------------------ every kernel, every shape
@pytest.mark.parametrize("si", range(len(R.SHAPES)), ids=[f"{a}x{b}" for a, b in R.SHAPES])
def test_attention_kernels_vs_float64(ops, si):
    Nq, Nk = R.SHAPES[si]
    fams, cases, q, k, v = launch_case(si)
    tag = f"[{Nq}x{Nk}]"
    judge(f"attention_f64/f32{tag}", run_f32(q, k, v, B0, H0, Nq, Nk), cases, fams, H0, Nq)
    o3 = ops.attention_bf3(ops.split_bf3(q), ops.split_bf3(k), ops.split_bf3(v), B0, H0, Nq, Nk)
    judge(f"attention_f64/bf3{tag}", bf3_value(o3), cases, fams, H0, Nq)
    q2, k2, v2 = ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v)
    for n in (2, 1):
        with form(n):
            o2 = run_fh2(ops, q2, k2, v2, B0, H0, Nq, Nk)
        judge(f"attention_f64/fh2_form{n}{tag}", o2.value().cpu().numpy(), cases, fams, H0, Nq, v_scale=1.0, out_scale=1.0)


@pytest.mark.parametrize("Nq,Nk", R.SINGLE_PASS_SHAPES)
def test_single_pass_mode_vs_float64_on_the_first_planes(ops, Nq, Nk):
    si = R.SHAPES.index((Nq, Nk))
    fams, cases, q, k, v = launch_case(si, single=(1.0, 1.0, 1.0))
    q2, k2, v2 = ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v)
    prev = ops.fh2_set_passes(1)
    try:
        assert prev == 3
        with form(2):
            o2 = run_fh2(ops, q2, k2, v2, B0, H0, Nq, Nk)
    finally:
        assert ops.fh2_set_passes(prev) == 1
    judge(f"attention_f64/fh2_single_pass[{Nq}x{Nk}]", o2.value().cpu().numpy(), cases, fams, H0, Nq, v_scale=1.0, out_scale=1.0)


@pytest.mark.parametrize("B,H", R.GROUP_COUNTS)
def test_group_counts(ops, B, H):
    """1, 7, 8, 9 and 17 (batch, head) groups with two query blocks each: the workgroups past the last group return early, and
    h = group % H, b = group / H holds for every H"""
    Nq, Nk = R.GROUP_SHAPE
    si = R.SHAPES.index((Nq, Nk))
    fams, cases, q, k, v = launch_case(si, B, H)
    with form(2):
        o2 = run_fh2(ops, ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B, H, Nq, Nk)
    judge(f"attention_f64/fh2_groups[{B}x{H}]", o2.value().cpu().numpy(), cases, fams, H, Nq, v_scale=1.0, out_scale=1.0)


# ------------------------------------------------------------------------------------------------------------ layouts and scales
def fused(q, k, v, B, Nq, Nk, with_q):
    """[B max(Nq, Nk), 3 D] (or [B Nk, 2 D] without q) with q, k, v as column blocks; q fills the first B Nq rows"""
    D = q.shape[1]
    rows = B * max(Nq, Nk) if with_q else B * Nk
    m = torch.zeros(rows, (3 if with_q else 2) * D, device="cuda")
    c = 0
    if with_q:
        m[:B * Nq, :D] = q
        c = D
    m[:B * Nk, c:c + D] = k
    m[:B * Nk, c + D:c + 2 * D] = v
    return m


def padded_launch(call, unit, out_rows, D, args):
    """a raw C call with ldo = D + 32 into a buffer of 0xA5 bytes with 16 guard bytes behind it -> the [rows, D] part as bytes;
    asserts that the extra columns and the guard are untouched.  unit: bytes per element of the packed form."""
    ldo = D + 32
    buf = torch.full((out_rows * ldo * unit + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    call(buf, ldo, *args)
    body = buf[:out_rows * ldo * unit].view(out_rows, ldo * unit)
    assert bool((body[:, D * unit:] == 0xA5).all()), "columns past D were written"
    assert bool((buf[out_rows * ldo * unit:] == 0xA5).all()), "the guard was written"
    return body[:, :D * unit].contiguous()


@pytest.mark.parametrize("Nq,Nk", R.LAYOUT_SHAPES)
def test_layouts(ops, Nq, Nk):
    """q, k, v as column slices of one matrix, k and v as slices of one, and a padded output pitch: the same bytes as the plain
    launch (which is judged against float64), every byte of the D columns written, nothing else touched"""
    lib = _lib.load()
    si = R.SHAPES.index((Nq, Nk))
    fams, cases, q, k, v = launch_case(si)
    D = H0 * 64
    qkv, kv = fused(q, k, v, B0, Nq, Nk, True), fused(q, k, v, B0, Nq, Nk, False)
    # ---- bf3
    o3 = ops.attention_bf3(ops.split_bf3(q), ops.split_bf3(k), ops.split_bf3(v), B0, H0, Nq, Nk)
    judge(f"attention_f64/bf3_layouts[{Nq}x{Nk}]", bf3_value(o3), cases, fams, H0, Nq)
    qkv3, kv3, q3 = ops.split_bf3(qkv), ops.split_bf3(kv), ops.split_bf3(q)
    assert torch.equal(ops.attention_bf3(qkv3, qkv3, qkv3, B0, H0, Nq, Nk, q_col=0, k_col=D, v_col=2 * D).data, o3.data)
    assert torch.equal(ops.attention_bf3(q3, kv3, kv3, B0, H0, Nq, Nk, k_col=0, v_col=D).data, o3.data)

    def call3(buf, ldo):
        _lib.check(lib.a3r_attention_bf3(p(qkv3.data), 3 * D, p(qkv3.data, D * 6), 3 * D, p(qkv3.data, 2 * D * 6), 3 * D, p(buf), ldo,
                                         B0, H0, Nq, Nk, 0, _lib.stream_ptr()), "attention_bf3")
    assert torch.equal(padded_launch(call3, 6, B0 * Nq, D, ()), o3.data.view(B0 * Nq, D * 6))
    # ---- fh2, both forms
    for n in (2, 1):
        with form(n):
            o2 = run_fh2(ops, ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B0, H0, Nq, Nk)
            judge(f"attention_f64/fh2_form{n}_layouts[{Nq}x{Nk}]", o2.value().cpu().numpy(), cases, fams, H0, Nq, v_scale=1.0, out_scale=1.0)
            qkv2, kv2, q2 = ops.split_fh2(qkv), ops.split_fh2(kv), ops.split_fh2(q)
            assert torch.equal(run_fh2(ops, qkv2, qkv2, qkv2, B0, H0, Nq, Nk, q_col=0, k_col=D, v_col=2 * D).data, o2.data)
            assert torch.equal(run_fh2(ops, q2, kv2, kv2, B0, H0, Nq, Nk, k_col=0, v_col=D).data, o2.data)
            word = ops.absmax_word("cuda")

            def call2(buf, ldo):
                r = _lib.Fh2AttnRange(1.0, 1.0, 1.0, 1.0, word.data_ptr())
                _lib.check(lib.a3r_attention_fh2(p(qkv2.data), 3 * D, p(qkv2.data, D * 4), 3 * D, p(qkv2.data, 2 * D * 4), 3 * D, p(buf), ldo,
                                                 B0, H0, Nq, Nk, C.byref(r), _lib.stream_ptr()), "attention_fh2")
            assert torch.equal(padded_launch(call2, 4, B0 * Nq, D, ()), o2.data.view(B0 * Nq, D * 4))
            check_statistic(ops, o2, word)


@pytest.mark.parametrize("Nq,Nk", R.LAYOUT_SHAPES)
def test_operand_scales(ops, Nq, Nk):
    """q, k x 2^-6 stored at scale 2^6, v x 2^-10 stored at 2^10 and the output written at 2^10: the same tol_i, which carries the
    scales.  The same inputs stored at scale 1 have subnormal second planes: they pass, and only through the 2^-25 floor term."""
    si = R.SHAPES.index((Nq, Nk))
    fams, cases, q, k, v = launch_case(si, mul=SCALED_MUL)
    qs, ks, vs, os_ = SCALED
    with form(2):
        o2 = run_fh2(ops, ops.split_fh2(q, qs), ops.split_fh2(k, ks), ops.split_fh2(v, vs), B0, H0, Nq, Nk, out_scale=os_)
        o1 = run_fh2(ops, ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B0, H0, Nq, Nk)
    assert o2.scale == os_
    judge(f"attention_f64/fh2_scaled[{Nq}x{Nk}]", o2.value().cpu().numpy(), cases, fams, H0, Nq, v_scale=vs, out_scale=os_)
    out1 = o1.value().cpu().numpy()
    judge(f"attention_f64/fh2_scaled_inputs_at_scale_1[{Nq}x{Nk}]", out1, cases, fams, H0, Nq, v_scale=1.0, out_scale=1.0)
    no_floor = max(float((c.row_errors(R.group_block(out1, g, H0, Nq)) / c.tol()).max()) for g, c in enumerate(cases))
    record_margin(f"attention_f64/fh2_scaled_inputs_at_scale_1_without_floor[{Nq}x{Nk}]", worst=no_floor)
    assert no_floor > 1.0, no_floor


# ------------------------------------------------------------------------------------------------------------ output statistic
def test_statistic_ignores_rows_past_nq(ops):
    """One q buffer of 40 rows whose last seven are sharp (near one-hot rows: outputs as large as single V rows), launched with
    Nq = 33 and with Nq = 40: the first 33 output rows are the same bytes, the word of the Nq = 33 launch is the maximum over those
    rows alone (its workgroup computes 128 query lanes, the ones past Nq from clamped rows), the word of the Nq = 40 launch is larger."""
    H, Nq, Nq2, Nk = 5, 33, 40, 97
    D = H * 64
    q, k, v = np.empty((Nq2, D), np.float32), np.empty((Nk, D), np.float32), np.empty((Nk, D), np.float32)
    for h in range(H):
        q[:, h * 64:(h + 1) * 64], k[:, h * 64:(h + 1) * 64], v[:, h * 64:(h + 1) * 64] = R.attn_inputs("plain", Nq2, Nk, 4242 + h)
    q[Nq:] *= 8.0
    ref = np.concatenate([R.attn_truth(q[:, h * 64:(h + 1) * 64], k[:, h * 64:(h + 1) * 64], v[:, h * 64:(h + 1) * 64])[0] for h in range(H)], 1)
    assert np.abs(ref[Nq:]).max() > 1.5 * np.abs(ref[:Nq]).max()                 # (host, float64: the later rows would move the word)
    q2, k2, v2 = ops.split_fh2(dev(q)), ops.split_fh2(dev(k)), ops.split_fh2(dev(v))
    for n in (2, 1):
        with form(n):
            wa, wb = ops.absmax_word("cuda"), ops.absmax_word("cuda")
            oa = ops.attention_fh2(q2, k2, v2, 1, H, Nq, Nk, out_absmax=wa)
            ob = ops.attention_fh2(q2, k2, v2, 1, H, Nq2, Nk, out_absmax=wb)
        a, b = check_statistic(ops, oa, wa), check_statistic(ops, ob, wb)
        assert torch.equal(oa.data.view(Nq, D * 4), ob.data.view(Nq2, D * 4)[:Nq])
        first = float(ob.value()[:Nq].abs().max())
        assert abs(a - first) <= R.U22 * first and b > 1.5 * a, (n, a, first, b)
