"""GPU: the memory-bound producers of csrc/elementwise.hip against float64, on every launcher branch and loop path.

LayerNorm in its three output forms, the bilinear 2x, the final 1x1 conv + postprocess, stand-alone RoPE-2D, patchify and the
gather-add.  The kernel forms of this file are pinned to each other bit for bit elsewhere (test_gpu_bf3.py, test_gpu_fh2.py,
test_gpu_up2x_forms.py, test_gpu_dedup*.py); here the FIRST form of each chain is compared with a plain float64 reference, with
tolerances that come from the number formats and from the reference's own fp32 evaluation (tests/producer_refs.py;
tests/test_producer_refs_cpu.py shows that fp32 arithmetic in the kernels' order meets them).  Outputs are pre-filled with NaN
(0xFF bytes for the packed forms: a NaN in every bf16 / fp16 plane) and must be fully written; rows and pixels never repeat.

Launcher branches (every hipLaunchKernelGGL of the entry points named in the left column) and the case that reaches each:

  a3r_layernorm        layernorm_kernel<4 | 3 | 1, fp32>        test_layernorm_f32 (81, 1024) | (83, 768) | (1, 256)
                       layernorm_generic_kernel<fp32>           test_layernorm_f32 (1, 4) (3, 36) (80, 100) (80, 1280) (5, 2052);
                                                                test_layernorm_bf3 (1, 8) (5, 40) (6, 32); test_layernorm_fh2 D = 32 ... 2048
  a3r_layernorm_bf3    layernorm_kernel<4 | 3 | 1, bf3>         test_layernorm_bf3 plain (1, 1024) | (9, 768) | (1, 256) (7, 256)
                       layernorm_pair_kernel<4 | 3 | 1>         test_layernorm_bf3 pair  (1, 1024) | (9, 768) | (1, 256) (7, 256)
                                                                (M odd: the last wave has a single row)
                       layernorm_generic_kernel<bf3>            test_layernorm_bf3 plain (1, 8) (5, 40) (80, 1280) (6, 32); pair (80, 1280) (6, 32)
  a3r_layernorm_fh2    layernorm_fh2_kernel<1, stats | none>    test_layernorm_fh2 D = 32, 64, 480, 512 (480: last lane group partly filled)
                       layernorm_fh2_kernel<2, stats | none>    test_layernorm_fh2 D = 544, 768, 1024
                       layernorm_fh2_kernel<3, stats | none>    test_layernorm_fh2 D = 1056, 1280, 1536
                       layernorm_generic_kernel<fh2>            test_layernorm_fh2 D = 1568, 2048; test_layernorm_fh2_unaligned (D = 256)
                       persistent row loop, second trip         test_layernorm_fh2_persistent (16391, 32): 4098 row blocks on 4096 workgroups
  a3r_upsample2x       upsample2x_kernel<fp32> (form 1)         test_upsample2x_f64, every shape; y loop second trip: B = 4100 and 7300
                       upsample2x_block_kernel<fp32> (form 2)   test_upsample2x_f64, every shape; y loop second trip: B = 7300
  a3r_upsample2x_bf3   upsample2x_kernel<bf3>                   test_upsample2x_bf3; y loop second trip: (4100, 8, 3, 8)
  a3r_upsample2x_fh2,  upsample2x_kernel<fh2 | combine>, upsample2x_block_kernel<fh2 | combine>: bitwise on the fp32
  .._combine_fh2       form in test_gpu_up2x_forms.py / test_gpu_fh2_range.py / test_gpu_dedup_head.py (not repeated here)
  a3r_head_final       head_final_kernel                        test_head_final (1, 8) (7, 36) (9, 132: j += 32 loop) (969, 256)
                       uniform trip loop, second trip           test_head_final (131085, 8)
                       head_final128_kernel                     test_head_final (31, 128): one partial step
                       uniform trip loop, second trip           test_head_final (262157, 128): last step partial
  a3r_rope2d           rope2d_kernel                            test_rope2d, every case; grid-stride second trip: (4, 4100, 16, 128)
  a3r_patchify         patchify_kernel                          test_patchify_past_the_grid_cap, both layouts: second trip
  a3r_gather_add_rows  gather_add_rows_kernel                   test_gather_add_rows_past_the_grid_cap, b given and null: second trip

Measured on an MI355X (worst error / its tolerance over the cases of an operator; every figure goes through conftest.record_margin):
  a3r_layernorm (fp32)   per family 4 max(e32, 2^-22 max|ref|)          0.42 of it (offset rows, D = 544: 3.9e-4 against 9.2e-4);
                                                                        plain 0.18, spike 0.21, tiny 0.06, const rows = b bitwise
  a3r_layernorm_fh2      that + 2^-21 |y| + 2^-24 / min(s, 1)           0.39 against float64, 0.55 against the fp32 kernel
  a3r_upsample2x         (2 (H + W) + 8) 2^-24 max|x_b|                 0.17 of it (1 x 300 x 3 x 4), both forms alike
  a3r_head_final         4 max(e32, 2^-22 max|ref|)                     pts 0.29 (1.5e-5 against 5.2e-5), conf 0.22 (5.5e-6 against 2.6e-5)
  a3r_rope2d             (4 pmax + 8) 2^-24 hypot(u, v)                 0.26 of it (pmax = 2000); forward then backward 0.008 of twice it
  bf3 forms, patchify, gather-add                                       bitwise
"""
import ctypes as C

import numpy as np
import pytest
import torch

import producer_refs as R
from conftest import record_margin
from align3r_amd import _lib
from test_gpu_up2x_forms import SHAPES as UP_FORM_SHAPES, both_forms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from align3r_amd import ops as o
    return o


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def sentinel(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")


def ln_f32(x, w, b):
    """a3r_layernorm into a NaN-filled output"""
    M, D = x.shape
    y = nan_like(M, D)
    _lib.check(_lib.load().a3r_layernorm(p(x), p(w), p(b), p(y), M, D, R.LN_EPS, _lib.stream_ptr()), "layernorm")
    assert not torch.isnan(y).any()
    return y


def check_ln_f64(name, y, x, w, b, fam):
    """y [M, D] (anything float64-convertible) against float64 per family; const rows equal b bit for bit when y is fp32"""
    tol, ref = R.ln_tolerances(x, w, b, fam)
    err = R.ln_family_errors(y, ref, fam)
    record_margin(name, **{R.FAMILIES[f]: (err[f], tol[f]) for f in err})
    for f in err:
        assert err[f] <= tol[f], (name, R.FAMILIES[f], err[f], tol[f])
    return tol, ref


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M,D", R.LN_F32_CASES)
def test_layernorm_f32(M, D):
    x, w, b, fam = R.ln_inputs(M, D, seed=M * 10000 + D)
    y = ln_f32(dev(x), dev(w), dev(b)).cpu().numpy()
    check_ln_f64(f"producers/layernorm[{M}x{D}]", y, x, w, b, fam)
    const = fam == R.FAMILIES.index("const")
    assert np.array_equal(y[const], np.broadcast_to(b, y[const].shape))


@pytest.mark.parametrize("M,D,pair", [(M, D, pair) for M, D in R.LN_BF3_CASES for pair in (False, True) if not (pair and D % 32)])
def test_layernorm_bf3(ops, M, D, pair):
    x, w, b, fam = R.ln_inputs(M, D, seed=M * 10000 + D + 1)
    xd, wd, bd = dev(x), dev(w), dev(b)
    y = ln_f32(xd, wd, bd)
    check_ln_f64(f"producers/layernorm[{M}x{D}]", y.cpu().numpy(), x, w, b, fam)
    rows = M + (M & 1) if pair else M
    buf = sentinel(rows * D * 6)
    _lib.check(_lib.load().a3r_layernorm_bf3(p(xd), p(wd), p(bd), p(buf), M, D, R.LN_EPS, int(pair), _lib.stream_ptr()), "layernorm_bf3")
    got = ops.Bf3(buf, rows, D, weight=pair).planes()
    assert torch.equal(got[:, :M], ops.split_bf3(y).planes())             # (a sentinel left in place is a NaN: not equal)
    if rows > M:
        assert torch.isnan(got[:, M]).all()                                # the missing partner of the last row is not written


def ln_fh2(ops, x, w, b, scale, word):
    M, D = x.shape
    buf = sentinel(M * D * 4)
    _lib.check(_lib.load().a3r_layernorm_fh2(p(x), p(w), p(b), p(buf), M, D, R.LN_EPS, float(scale), p(word), _lib.stream_ptr()), "layernorm_fh2")
    return ops.Fh2(buf, M, D, scale)


def check_ln_fh2(ops, name, x, w, b, fam, xd=None):
    """a3r_layernorm_fh2 with and without a statistics word at scales 1 and 2^-5: fully written, the same bits with and without
    the word, inside the float64 tolerance plus the format's resolution, near the fp32 kernel, const rows = split of b scale,
    word = max |stored|."""
    M, D = x.shape
    wd, bd = dev(w), dev(b)
    xa = dev(x)
    xd = xa if xd is None else xd
    y32 = ln_f32(xa, wd, bd).double()
    tol, ref = check_ln_f64(f"{name}/f32", y32.cpu().numpy(), x, w, b, fam)
    tol_rows = torch.tensor([tol[int(f)] for f in fam], dtype=torch.float64, device="cuda")[:, None]
    refd = dev(ref)
    const = torch.from_numpy(fam == R.FAMILIES.index("const")).cuda()
    for scale in (1.0, 2.0 ** -5):
        word = ops.absmax_word("cuda")
        with_word, without = ln_fh2(ops, xd, wd, bd, scale, word), ln_fh2(ops, xd, wd, bd, scale, None)
        planes = with_word.planes()
        assert not torch.isnan(planes).any()
        assert torch.equal(with_word.data, without.data)
        v = with_word.value()
        res64, res32 = R.fh2_resolution(refd, scale), R.fh2_resolution(y32, scale)
        e64, e32 = (v - refd).abs(), (v - y32).abs()
        record_margin(f"{name}/fh2[s={scale:g}]", vs_f64=float((e64 / (tol_rows + res64)).max()), vs_f32_kernel=float((e32 / (tol_rows + res32)).max()))
        assert bool((e64 <= tol_rows + res64).all()), (name, scale, float((e64 / (tol_rows + res64)).max()))
        assert bool((e32 <= tol_rows + res32).all()), (name, scale, float((e32 / (tol_rows + res32)).max()))
        if bool(const.any()):
            n = int(const.sum())
            want = ops.split_fh2((bd * scale)[None, :].expand(n, D).contiguous())
            assert torch.equal(with_word.data.view(M, 4 * D)[const], want.data.view(n, 4 * D))
        stored = float((planes[0].double() + planes[1].double()).abs().max())
        assert abs(ops.absmax_value(word) - stored) <= 2.0 ** -21 * stored + 2.0 ** -24, (ops.absmax_value(word), stored)


@pytest.mark.parametrize("D", R.LN_FH2_D)
def test_layernorm_fh2(ops, D):
    M = R.LN_FH2_M
    x, w, b, fam = R.ln_inputs(M, D, seed=M * 10000 + D + 2)
    check_ln_fh2(ops, f"producers/layernorm_fh2[{M}x{D}]", x, w, b, fam)


def test_layernorm_fh2_unaligned(ops):
    """x a contiguous view 4 bytes into a larger buffer: the launcher must take the generic kernel (no 16-byte loads)"""
    M, D = R.LN_FH2_M, R.LN_FH2_UNALIGNED_D
    x, w, b, fam = R.ln_inputs(M, D, seed=M * 10000 + D + 3)
    big = torch.zeros(M * D + 8, device="cuda")
    xd = big[1:1 + M * D].view(M, D)
    xd.copy_(dev(x))
    assert big.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    check_ln_fh2(ops, f"producers/layernorm_fh2_unaligned[{M}x{D}]", x, w, b, fam, xd=xd)


def test_layernorm_fh2_persistent(ops):
    """more row blocks than the 4096 workgroups a launch with statistics gets: workgroups 0 and 1 take a second trip.  (Without
    the word the launch has one workgroup per block: the two outputs must be the same bits.)"""
    M, D = R.LN_FH2_PERSISTENT
    assert (M + 3) // 4 > 4096
    x, w, b, fam = R.ln_inputs(M, D, seed=M * 10000 + D + 4)
    check_ln_fh2(ops, f"producers/layernorm_fh2_persistent[{M}x{D}]", x, w, b, fam)


# ------------------------------------------------------------------------------------------------------------ bilinear 2x
@pytest.mark.parametrize("B,H,W,Cc,crop", UP_FORM_SHAPES + R.UP_EXTRA)
def test_upsample2x_f64(B, H, W, Cc, crop):
    x = R.up_input(B, H, W, Cc, seed=H * 100 + W)
    ref, tol = dev(R.up_ref64(x, crop)), dev(R.up_tolerance(x))
    xd = dev(x)
    Hc, Wc = crop if crop else (2 * H, 2 * W)

    def run():
        out = nan_like(B, Hc, Wc, Cc)
        _lib.check(_lib.load().a3r_upsample2x(p(xd), p(out), B, H, W, Cc, Hc, Wc, _lib.stream_ptr()), "upsample2x")
        return out
    worst = []
    for form, out in zip((1, 2), both_forms(run)):
        assert not torch.isnan(out).any(), form
        ratio = float(((out.double() - ref).abs() / tol).max())
        worst.append(ratio)
    record_margin(f"producers/upsample2x[{B}x{H}x{W}x{Cc},{crop}]", form1=worst[0], form2=worst[1], tol=float(tol.max()))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("B,H,W,Cc,crop", R.UP_BF3)
def test_upsample2x_bf3(ops, B, H, W, Cc, crop):
    x = R.up_input(B, H, W, Cc, seed=H * 100 + W + 1)
    xd = dev(x)
    y = ops.upsample2x(xd, crop=crop)
    assert bool(((y.double() - dev(R.up_ref64(x, crop))).abs() <= dev(R.up_tolerance(x))).all())
    got = ops.upsample2x_bf3(xd, crop=crop)
    assert (got.rows, got.K) == (y.numel() // Cc, Cc)
    assert torch.equal(got.planes(), ops.split_bf3(y).planes())           # (an unwritten pixel is three zero planes: not equal)


# ------------------------------------------------------------------------------------------------------------ head final
@pytest.mark.parametrize("P,Cc", R.HEAD_CASES)
def test_head_final(P, Cc):
    x, w, bias = R.head_inputs(P, Cc, seed=P + Cc)
    zero_pix = P // 2
    x0 = x.clone()
    x0[zero_pix] = 0
    wd = w.cuda()
    for name, xv, bv in (("bias", x, bias), ("zero", x0, torch.zeros(4))):
        p64, c64, tol_p, tol_c, dmax, f3max = R.head_refs(xv, w, bv)
        assert dmax < 6 and f3max < 6, (dmax, f3max)                      # beyond that expm1's growth, not the kernel, sets the error
        xd, bd = xv.cuda(), bv.cuda()
        pts, conf = nan_like(P, 3), nan_like(P)
        _lib.check(_lib.load().a3r_head_final(p(xd), p(wd), p(bd), p(pts), p(conf), P, Cc, _lib.stream_ptr()), "head_final")
        pts, conf = pts.cpu(), conf.cpu()
        assert not torch.isnan(pts).any() and not torch.isnan(conf).any()
        ep, ec = float((pts.double() - p64).abs().max()), float((conf.double() - c64).abs().max())
        record_margin(f"producers/head_final[{P}x{Cc},{name}]", pts=(ep, tol_p), conf=(ec, tol_c))
        assert ep <= tol_p and ec <= tol_c, (name, ep, tol_p, ec, tol_c)
        if name == "zero":
            assert bool((pts[zero_pix] == 0).all()) and float(conf[zero_pix]) == 2.0


# ------------------------------------------------------------------------------------------------------------ RoPE-2D
@pytest.mark.parametrize("B,N,H,D,pmax", R.ROPE_CASES)
def test_rope2d(ops, B, N, H, D, pmax):
    tok, pos = R.rope_inputs(B, N, H, D, pmax, seed=D + pmax)
    tokd, posd = tok.cuda(), pos.cuda()
    tol = R.rope_tolerance(tokd, pmax)
    worst = {}
    for fwd in (1.0, -1.0):
        ref = R.rope_ref64(tokd, posd, fwd)
        got = ops.rope_2d(tokd.clone(), posd, R.ROPE_BASE, fwd)
        e = (got.double() - ref).abs()
        worst[f"fwd={fwd:+g}"] = float((e / tol.clamp(min=1e-300)).max())
        assert bool((e <= tol).all()), (fwd, worst)
        del ref, e
        if fwd == 1.0:                                                      # forward then backward returns the input
            back = ops.rope_2d(got, posd, R.ROPE_BASE, -1.0)
            e = (back.double() - tokd.double()).abs()
            worst["round_trip/2"] = float((e / (2 * tol).clamp(min=1e-300)).max())
            assert bool((e <= 2 * tol).all()), worst
            del back, e
    record_margin(f"producers/rope2d[{B}x{N}x{H}x{D},pmax={pmax}]", **worst)


# ------------------------------------------------------------------------------------------------------------ grid-stride copies
@pytest.mark.parametrize("channels_last", [False, True])
def test_patchify_past_the_grid_cap(channels_last):
    B, Cc, H, W = R.PATCHIFY_SHAPE
    assert B * Cc * H * W > 65536 * 256
    g = torch.Generator(device="cuda").manual_seed(11)
    img = torch.randn(B, Cc, H, W, device="cuda", generator=g)
    ref = img.reshape(B, Cc, H // 16, 16, W // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, Cc * 256)
    if channels_last:
        src, strides = img.permute(0, 2, 3, 1).contiguous(), (H * W * Cc, 1, W * Cc, Cc)
    else:
        src, strides = img, (Cc * H * W, H * W, W, 1)
    cols = nan_like(*ref.shape)
    _lib.check(_lib.load().a3r_patchify(p(src), p(cols), B, Cc, H, W, *strides, _lib.stream_ptr()), "patchify")
    assert torch.equal(cols, ref)


@pytest.mark.parametrize("in_place", [False, True])
def test_gather_add_rows_past_the_grid_cap(in_place):
    S, N, Cc, Ua, Ub = R.GATHER_ADD_SHAPE
    assert S * N * (Cc // 4) > 65536 * 256
    g = torch.Generator(device="cuda").manual_seed(12)
    a = torch.randn(Ua, N, Cc, device="cuda", generator=g)
    ma = torch.tensor(R.GATHER_MAP_A, dtype=torch.int32, device="cuda")
    if in_place:
        dst = torch.randn(S, N, Cc, device="cuda", generator=g)
        ref = dst + a[ma.long()]
        b = mb = None
    else:
        b = torch.randn(Ub, N, Cc, device="cuda", generator=g)
        mb = torch.tensor(R.GATHER_MAP_B, dtype=torch.int32, device="cuda")
        dst = nan_like(S, N, Cc)
        ref = a[ma.long()] + b[mb.long()]
    _lib.check(_lib.load().a3r_gather_add_rows(p(a), p(ma), p(b), p(mb), p(dst), S, N, Cc, _lib.stream_ptr()), "gather_add_rows")
    assert torch.equal(dst, ref)
