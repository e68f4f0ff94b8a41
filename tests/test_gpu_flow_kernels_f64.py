"""GPU: the flow network's kernels that have no GEMM shape (csrc/raft.hip) against float64, on every launcher branch and loop path.

The operator entries a3r_flow_* go through the launch_* functions the plan of a3r_raft_forward uses, so the grid a case runs is
production's.  References, restatements and tolerances are in tests/flow_refs.py (derived from the formats and the operation
counts; tests/test_flow_refs_cpu.py shows that fp32 in the kernels' order uses at most half of each, that the references agree
where two routes exist, that the input families reach what they are there for, and that every bound sees the fault it is there
for).  Outputs are pre-filled with NaN and must be fully written; every margin goes through conftest.record_margin.

Launcher branches (every hipLaunchKernelGGL of the kernel section of csrc/raft.hip) and the case that reaches each:

  launch_direct_conv   direct_conv_fixed_kernel<7, 2, 8>        test_stem_f64: 8x8, 24x40 (Wo = 20: a thread with 4 of 8 columns), 16x16,
                                                                40x56 (Wo = 28); one and two sources, Cout 32 / 64, B 1 / 2, relu on / off
                       .. grid-stride second trip               test_stem_past_the_grid_cap (1 x 2048 x 4112, Cout 64: 2^24 + 65536 threads)
                       direct_conv_fixed_kernel<7, 1, 8>        test_flow_conv_f64: 2x2, 5x7, 16x20, 22x21, Cout 64 / 128, |flow| up to 100
                       direct_conv_kernel (form 1)              the same cases of both tests, bitwise the fixed form
                       .. through A3R_RAFT_DIRECT_CONV=generic  NOT reached: the variable is read once per process, so it needs a child
                                                                process; it selects the same launch line as form 1
                       .. with k != 7 or another stride         NOT reached: no caller; the plan and the entries fix k = 7, stride 1 or 2
                       .. second trip, stride 1 or generic      NOT reached: convf1 at 48 pairs of 384x512 is 2.4 M threads, and the generic
                                                                kernel is an A/B form; the loop is the one line the stride-2 case runs
  launch_transpose     transpose_kernel                         every convolution case (the entries transpose the weights as finalize does)
  launch_dwconv7       dwconv7_kernel                           test_dwconv7_f64: 1x1, 3x5, 16x20, 22x21, 9x42 (w % 4 = 0, 1, 2; h < 7), C 192 / 384
                       .. grid-stride second trip               test_dwconv7_past_the_grid_cap (16 x 64 x 172 x 384: 2^24 + 131072 threads)
  launch_gather_s2     gather_s2_kernel                         test_gather_and_halve: 2x2, 5x5, 22x21, 9x7, C 128 / 256
                       .. grid-stride second trip               test_gather_s2_past_the_grid_cap (8 x 513 x 257 x 256)
  launch_halve         halve_kernel                             test_gather_and_halve, the same shapes (odd sizes drop the last row / column)
                       .. grid-stride second trip               NOT reached: 9.4 M threads at 48 pairs of 384x512, 0.56 of the cap
  launch_corr_lookup   corr_lookup_kernel                       test_corr_lookup_f64: r 2 / 4 with 4 levels, r 4 with 2, maps 16x20 and 22x21,
                                                                ldo = channels, + 1, padded to 32; five target families in every call
                       .. grid-stride second trip               test_corr_lookup_past_the_grid_cap (187 x 16 x 16, r 4, ldo 352)
  launch_convex_upsample  convex_upsample_kernel                test_convex_upsample_f64: 2x2, 2x3, 16x20, 22x21; four logit families
                       .. grid-stride second trip               NOT reached: 9.4 M threads at 48 pairs of 384x512, 0.56 of the cap
  launch_scale         scale_kernel                             test_movers; second trip: test_movers_past_the_grid_cap (2^24 + 12345)
  launch_pack_cols     pack_cols_kernel                         test_movers; second trip: test_movers_past_the_grid_cap (38927 x 431)
  launch_flow_add      flow_add_kernel                          test_movers
                       .. grid-stride second trip               NOT reached: 2 Bhw = 0.3 M threads at 48 pairs of 384x512
  launch_image_absmax  image_absmax_kernel                      test_image_absmax: n_per below and above 64 x 1024 (one trip / the loop), a single
                                                                maximum in the last element, a negative maximum

Measured on an MI355X (worst error / its tolerance over the cases of an operator; every figure goes through conftest.record_margin):
  stems, fixed form          (n + 2) U (sum |x^||w| + |b|) + normalisation    0.064 (24x40, one source, Cout 64); past the cap 0.018
  convf1, fixed form         (n + 2) U (sum |x||w| + |b|)                     0.19 (2x2, Cout 128)
  generic against fixed      both strides, every case                         bitwise
  depthwise 7x7              (n + 2) U (sum |x||w| + |b|)                     0.32 (1x1, C 384: a one-tap chain); past the cap 0.054
  halve                      4 U max |block|                                  0.32 (22x21, C 256); bitwise the fp32 restatement
  lookup                     coordinate chain x Lipschitz + 8 U sum |taps|    inside 0.28, integral 0.19, border 0.27, exact 0.26 (worst: 16x20,
                                                                              r 4, 4 levels); outside and padding exactly zero; past the cap 0.14
  convex up-sampling         2 U sum p |8 f| (|a| + A + 4 EXPF_ULPS + 20)     border cells 0.28 (16x20, near one-hot), interior 0.096
  gather_s2, pack_cols, scale, flow_add, image_absmax                         bitwise, past the cap included
  (U = 2^-24; tests/flow_refs.py has each derivation)
"""
import numpy as np
import pytest
import torch

import flow_refs as R
from conftest import record_margin

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from align3r_amd import ops as o
    return o


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def written(t):
    assert not torch.isnan(t).any()
    return t.cpu().numpy()


def check(name, got, ref, tol):
    """|got - ref| <= tol everywhere; records and returns the worst ratio"""
    ratio = float((np.abs(got.astype(np.float64) - ref) / tol).max())
    record_margin(name, err_over_tol=ratio)
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------ 7x7 direct convolutions
@pytest.mark.parametrize("H,W,two,Cout,B,relu", R.STEM_CASES)
def test_stem_f64(ops, H, W, two, Cout, B, relu):
    x0, x1, w, b = R.stem_inputs(H, W, two, Cout, B, seed=H * 1000 + W + Cout)
    ref, tol = R.conv7_ref64(R.stem_planes(x0, x1), w, b, 2, relu, R.IN_MUL, R.IN_ADD)
    args = (dev(x0), dev(w), dev(b), dev(x1), float(R.IN_MUL), float(R.IN_ADD), relu)
    fixed = ops.flow_conv7_planes(*args, form=0, out=nan_like(*ref.shape))
    generic = ops.flow_conv7_planes(*args, form=1, out=nan_like(*ref.shape))
    check(f"flow_kernels/stem[{H}x{W},{'two' if two else 'one'},{Cout},B{B},relu{int(relu)}]", written(fixed), ref, tol)
    assert torch.equal(fixed, generic)
    nobias = ops.flow_conv7_planes(args[0], args[1], None, *args[3:], form=0, out=nan_like(*ref.shape))
    assert torch.equal(nobias, ops.flow_conv7_planes(args[0], args[1], torch.zeros_like(args[2]), *args[3:], form=1))


@pytest.mark.parametrize("h,w,Cout,relu", R.CONVF_CASES)
def test_flow_conv_f64(ops, h, w, Cout, relu):
    flow, wt, b = R.convf_inputs(h, w, Cout, seed=h * 100 + w + Cout)
    ref, tol = R.conv7_ref64(np.ascontiguousarray(flow.transpose(0, 3, 1, 2)), wt, b, 1, relu)
    fixed = ops.flow_conv7_flow(dev(flow), dev(wt), dev(b), relu, form=0, out=nan_like(*ref.shape))
    generic = ops.flow_conv7_flow(dev(flow), dev(wt), dev(b), relu, form=1, out=nan_like(*ref.shape))
    check(f"flow_kernels/convf[{h}x{w},{Cout},relu{int(relu)}]", written(fixed), ref, tol)
    assert torch.equal(fixed, generic)


def subset_check(name, out, rows, ref, tol):
    got = out[tuple(torch.from_numpy(rows.T).cuda())].cpu().numpy()
    return check(name, got, ref, tol)


def test_stem_past_the_grid_cap(ops):
    """2^24 + 65536 threads: the last 65536 work items are second trips.  float64 on the first and last item and 256 either side of
    2^24 (every column those items own); the whole output finite."""
    B, H, W, Cout = R.STEM_CAP
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand(B, 3, H, W, device="cuda", generator=g) * 255
    w, b = (0.1 * torch.randn(Cout, 3, 7, 7, device="cuda", generator=g)), 0.5 * torch.randn(Cout, device="cuda", generator=g)
    Ho, Wo = H // 2, W // 2
    total = B * Ho * ((Wo + 7) // 8) * Cout
    out = ops.flow_conv7_planes(x, w, b, None, float(R.IN_MUL), float(R.IN_ADD), True, out=nan_like(B, Ho, Wo, Cout))
    assert torch.isfinite(out).all()
    rows, ref, tol = R.stem_ref64_at(lambda kb, y0, y1, x0, x1: x[kb, :, y0:y1, x0:x1].cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(), H, W,
                                     R.cap_items(total), True, R.IN_MUL, R.IN_ADD)
    assert len(rows) >= 8 * 514
    subset_check("flow_kernels/stem_past_cap", out, rows, ref, tol)


# ------------------------------------------------------------------------------------------------------------ depthwise 7x7
@pytest.mark.parametrize("h,w,C", R.DW_CASES)
def test_dwconv7_f64(ops, h, w, C):
    x, wt, b = R.dw_inputs(h, w, C, seed=h * 100 + w + C)
    ref, tol = R.dw_ref64(x, wt, b)
    out = ops.flow_dwconv7(dev(x), dev(wt), dev(b), out=nan_like(*x.shape))
    check(f"flow_kernels/dwconv7[{h}x{w},{C}]", written(out), ref, tol)


def test_dwconv7_past_the_grid_cap(ops):
    B, h, w, C = R.DW_CAP
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(B, h, w, C, device="cuda", generator=g)
    wt, b = 0.2 * torch.randn(C, 49, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    out = ops.flow_dwconv7(x, wt, b, out=nan_like(B, h, w, C))
    assert torch.isfinite(out).all()
    rows, ref, tol = R.dw_ref64_at(lambda kb, y0, y1, x0, x1: x[kb, y0:y1, x0:x1].cpu().numpy(), wt.cpu().numpy(), b.cpu().numpy(), (B, h, w, C),
                                   R.cap_items(B * h * ((w + 3) // 4) * C))
    assert len(rows) >= 4 * 513
    subset_check("flow_kernels/dwconv7_past_cap", out, rows, ref, tol)


# ------------------------------------------------------------------------------------------------------------ gather_s2, halve
@pytest.mark.parametrize("h,w,C", R.GH_CASES)
def test_gather_and_halve(ops, h, w, C):
    x = R.gh_input(h, w, C, seed=h * 10 + w)
    xd = dev(x)
    got = written(ops.flow_gather_s2(xd, out=nan_like(2, (h + 1) // 2, (w + 1) // 2, C)))
    assert np.array_equal(got.astype(np.float64), R.gather_ref(x))
    ref, tol = R.halve_ref64(x)
    half = written(ops.flow_halve(xd, out=nan_like(2, h // 2, w // 2, C)))
    assert np.array_equal(half, R.halve_restated(x))                        # .5 a + .5 b is one rounding whether or not it contracts
    check(f"flow_kernels/halve[{h}x{w},{C}]", half, ref, tol)


def test_gather_s2_past_the_grid_cap(ops):
    B, h, w, C = R.GATHER_CAP
    x = torch.randn(B, h, w, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13))
    out = ops.flow_gather_s2(x, out=nan_like(B, (h + 1) // 2, (w + 1) // 2, C))
    assert out.numel() // 4 > R.CAP
    assert torch.equal(out, x[:, ::2, ::2])


# ------------------------------------------------------------------------------------------------------------ correlation lookup
@pytest.mark.parametrize("h,w", R.LK_MAPS)
@pytest.mark.parametrize("r,levels", R.LK_CONFIGS)
def test_corr_lookup_f64(ops, h, w, r, levels):
    corr, qx, qy, flow, fam = R.lk_inputs(h, w, r, levels, seed=h * 100 + w + 10 * r + levels)
    ref, tol = R.lookup_ref64(corr, qx, qy, flow, r), R.lookup_tol(corr, qx, qy, flow, r)
    cd, fd = [dev(c) for c in corr], dev(flow.reshape(2, h, w, 2))
    nch, worst = ref.shape[1], {}
    for ldo in R.lk_ldos(r, levels):
        out = written(ops.flow_corr_lookup(cd, fd, r, ldo=ldo, out=nan_like(len(qx), ldo)))
        assert not out[:, nch:].any()                                       # the padding columns are exactly zero
        assert not out[fam == R.LK_FAMILIES.index("outside")].any()         # whole windows outside the map: exactly zero
        ratio = np.abs(out[:, :nch].astype(np.float64) - ref) / tol
        for k, name in enumerate(R.LK_FAMILIES):
            worst[name] = max(worst.get(name, 0.0), float(ratio[fam == k].max()))
    record_margin(f"flow_kernels/lookup[{h}x{w},r{r},L{levels}]", **worst)
    assert max(worst.values()) <= 1.0, worst


def test_corr_lookup_past_the_grid_cap(ops):
    """187 x 16 x 16 queries of 352 columns: 2^24 + 74496 work items.  float64 on every channel of the queries that hold the first and
    last item and the 512 around 2^24; the whole output finite, the padding columns zero."""
    B, h, w, r, levels, ldo = R.LK_CAP
    g = torch.Generator(device="cuda").manual_seed(14)
    Q = B * h * w
    corr = [torch.randn(Q, hl, wl, device="cuda", generator=g) for hl, wl in R.lk_levels(h, w, levels)]
    flow = 12 * torch.rand(B, h, w, 2, device="cuda", generator=g) - 6
    out = ops.flow_corr_lookup(corr, flow, r, ldo=ldo, out=nan_like(Q, ldo))
    nch = levels * (2 * r + 1) ** 2
    assert torch.isfinite(out).all() and not out[:, nch:].any()
    items = R.cap_items(Q * ldo)
    q = np.unique(items // ldo)
    assert {0, Q - 1, R.CAP // ldo} <= set(q.tolist())
    qd = torch.from_numpy(q).cuda()
    sub = [c[qd].cpu().numpy() for c in corr]
    fl = flow.reshape(Q, 2)[qd].cpu().numpy()
    args = (sub, q % w, (q // w) % h, fl, r)
    check("flow_kernels/lookup_past_cap", out[qd, :nch].cpu().numpy(), R.lookup_ref64(*args), R.lookup_tol(*args))


def test_corr_lookup_refuses_a_level_below_2x2(ops):
    flow = torch.zeros(1, 4, 4, 2, device="cuda")
    corr = [torch.zeros(16, 4, 4, device="cuda"), torch.zeros(16, 2, 1, device="cuda")]
    with pytest.raises(RuntimeError, match="smaller than 2x2"):
        ops.flow_corr_lookup(corr, flow, 2)
    with pytest.raises(RuntimeError, match="ldo"):
        ops.flow_corr_lookup(corr[:1], flow, 2, ldo=24)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.flow_gather_s2(torch.zeros(1, 2, 2, 6, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ convex up-sampling
@pytest.mark.parametrize("h,w", R.UP_SHAPES)
@pytest.mark.parametrize("family", R.UP_FAMILIES)
def test_convex_upsample_f64(ops, h, w, family):
    flow, mask = R.up_inputs(h, w, family, seed=h * 100 + w)
    ref, tol = R.up_ref64(flow, mask), R.up_tol(flow, mask)
    out = written(ops.flow_convex_upsample(dev(flow), dev(mask), out=nan_like(*ref.shape)))
    ratio = np.abs(out.astype(np.float64) - ref) / tol
    edge = R.up_border_pixels(h, w)
    record_margin(f"flow_kernels/convex_upsample[{h}x{w},{family}]", border=float(ratio[:, :, edge].max()),
                  interior=float(ratio[:, :, ~edge].max()) if (~edge).any() else 0.0)
    assert ratio.max() <= 1.0, float(ratio.max())


# ------------------------------------------------------------------------------------------------------------ the movers
def test_movers(ops):
    rng = np.random.default_rng(3)
    for rows, ldd, c0, lds, Cs in R.PACK_CASES:
        dst, src = rng.standard_normal((rows, ldd)).astype(F32), rng.standard_normal((rows, lds)).astype(F32)
        got = ops.flow_pack_cols(dev(dst), c0, dev(src), Cs).cpu().numpy()
        assert np.array_equal(got, R.pack_restated(dst, c0, src, Cs))       # the other columns of dst untouched
    s = F32(1.0 / np.sqrt(256.0) * 1.0000001)
    for n in R.SCALE_CASES:
        x = rng.standard_normal(n).astype(F32)
        assert np.array_equal(ops.flow_scale(dev(x), float(s)).cpu().numpy(), x * s)
    for rows, ldu in R.ADD_CASES:
        flow, upd = rng.standard_normal((rows, 2)).astype(F32), rng.standard_normal((rows, ldu)).astype(F32)
        assert np.array_equal(ops.flow_add(dev(flow), dev(upd)).cpu().numpy(), flow + upd[:, :2])


def test_movers_past_the_grid_cap(ops):
    """pack_cols and scale with more than 2^24 elements, bitwise on the whole array"""
    rows, ldd, c0, lds, Cs = R.PACK_CAP
    g = torch.Generator(device="cuda").manual_seed(15)
    dst, src = torch.randn(rows, ldd, device="cuda", generator=g), torch.randn(rows, lds, device="cuda", generator=g)
    want = dst.clone()
    want[:, c0:c0 + Cs] = src[:, :Cs]
    assert torch.equal(ops.flow_pack_cols(dst, c0, src, Cs), want)
    x = torch.randn(R.SCALE_CAP, device="cuda", generator=g)
    s = F32(0.0625 * 1.0000001)
    want = x.cpu().numpy() * s
    assert np.array_equal(ops.flow_scale(x, float(s)).cpu().numpy(), want)


@pytest.mark.parametrize("images,n_per", R.ABSMAX_CASES)
def test_image_absmax(ops, images, n_per):
    x = R.absmax_inputs(images, n_per, seed=n_per)
    got = ops.flow_image_absmax(dev(x)).cpu().numpy()
    assert np.array_equal(got, np.abs(x).max(axis=1))
