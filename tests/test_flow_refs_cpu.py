"""CPU: the fp32 arithmetic of the flow network's kernels without a GEMM shape (csrc/raft.hip), restated in numpy in the kernels' own
order, uses at most HALF of every tolerance tests/test_gpu_flow_kernels_f64.py asserts, at every shape and family that test uses --
the device, which may contract multiply-adds differently, then has room, and a failure there means a kernel computes something
else.  Also: the float64 references agree where two routes exist; the input families reach what they are there for (the
conditions of the GPU test's cases); and every tolerance sees the fault it is there for, shown once per operator on a
deliberately wrong restatement."""
import numpy as np
import pytest

import flow_refs as R

F32 = np.float32


def worst(got, ref, tol):
    return float((np.abs(got.astype(np.float64) - ref) / tol).max())


def split_ok(y, relu):
    """relu on: at least 20 % of the outputs clipped and at least 20 % kept"""
    if relu:
        z = float((y == 0).mean())
        assert 0.2 <= z <= 0.8, z


# ------------------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("H,W,two,Cout,B,relu", R.STEM_CASES)
def test_stem_restatement_uses_half_the_bound(H, W, two, Cout, B, relu):
    x0, x1, w, b = R.stem_inputs(H, W, two, Cout, B, seed=H * 1000 + W + Cout)
    x = R.stem_planes(x0, x1)
    ref, tol = R.conv7_ref64(x, w, b, 2, relu, R.IN_MUL, R.IN_ADD)
    got = R.conv7_restated(x, w, b, 2, relu, R.IN_MUL, R.IN_ADD)
    assert got.shape == ref.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout)
    assert worst(got, ref, tol) <= 0.5
    split_ok(ref, relu)


@pytest.mark.parametrize("h,w,Cout,relu", R.CONVF_CASES)
def test_flow_conv_restatement_uses_half_the_bound(h, w, Cout, relu):
    flow, wt, b = R.convf_inputs(h, w, Cout, seed=h * 100 + w + Cout)
    assert np.abs(flow).max() == R.FLOW_MAX
    x = np.ascontiguousarray(flow.transpose(0, 3, 1, 2))
    ref, tol = R.conv7_ref64(x, wt, b, 1, relu)
    assert worst(R.conv7_restated(x, wt, b, 1, relu), ref, tol) <= 0.5
    split_ok(ref, relu)


def test_stem_bound_sees_a_one_column_shift_in_the_ragged_tail():
    """24 x 40: Wo = 20, the last thread of a row owns columns 16..19.  Those four columns computed from the image one column to the
    left: every one of them leaves the bound."""
    x0, x1, w, b = R.stem_inputs(24, 40, False, 32, 1, seed=24040 + 32)
    ref, tol = R.conv7_ref64(x0, w, b, 2, False, R.IN_MUL, R.IN_ADD)
    wrong = R.conv7_restated(x0, w, b, 2, False, R.IN_MUL, R.IN_ADD)
    wrong[:, :, 16:] = R.conv7_restated(np.roll(x0, 1, axis=3), w, b, 2, False, R.IN_MUL, R.IN_ADD)[:, :, 16:]
    bad = np.abs(wrong - ref) > tol
    assert not bad[:, :, :16].any() and bad[:, :, 16:].mean() > 0.99


@pytest.mark.parametrize("h,w,C", R.DW_CASES)
def test_depthwise_restatement_uses_half_the_bound(h, w, C):
    x, wt, b = R.dw_inputs(h, w, C, seed=h * 100 + w + C)
    ref, tol = R.dw_ref64(x, wt, b)
    assert worst(R.dw_restated(x, wt, b), ref, tol) <= 0.5


def test_depthwise_bound_sees_a_one_column_shift_in_the_ragged_tail():
    """22 x 21: the last thread of a row owns column 20 alone (w % 4 = 1); 9 x 42: columns 40, 41 (w % 4 = 2)"""
    for h, w in ((22, 21), (9, 42)):
        x, wt, b = R.dw_inputs(h, w, 192, seed=h * 100 + w + 192)
        ref, tol = R.dw_ref64(x, wt, b)
        t0 = w - w % 4
        wrong = R.dw_restated(x, wt, b)
        wrong[:, :, t0:] = R.dw_restated(np.roll(x, 1, axis=2), wt, b)[:, :, t0:]
        bad = np.abs(wrong - ref) > tol
        assert not bad[:, :, :t0].any() and bad[:, :, t0:].mean() > 0.99


def test_depthwise_subset_reference_is_the_full_one():
    """dw_ref64_at (what the past-the-cap case uses) against dw_ref64 on a small map, every item; and the cap case's arithmetic"""
    shape = (2, 9, 42, 8)
    x, wt, b = R.dw_inputs(9, 42, 8, seed=5)
    ref, tol = R.dw_ref64(x, wt, b)
    items = np.arange(2 * 9 * 11 * 8)
    rows, y, t = R.dw_ref64_at(lambda kb, y0, y1, x0, x1: x[kb, y0:y1, x0:x1], wt, b, shape, items)
    assert len(rows) == x.size
    assert np.abs(y - ref[tuple(rows.T)]).max() <= 1e-13 and (t >= tol[tuple(rows.T)]).all()
    B, h, w, C = R.DW_CAP
    total = B * h * ((w + 3) // 4) * C
    assert total > R.CAP >= (B - 1) * h * ((w + 3) // 4) * C
    it = R.cap_items(total)
    assert it[0] == 0 and it[-1] == total - 1 and {R.CAP - 256, R.CAP - 1, R.CAP, R.CAP + 255} <= set(it.tolist())


def test_stem_subset_reference_is_the_full_one():
    """stem_ref64_at (what the past-the-cap case uses) against conv7_ref64 on a small image, every item; the cap cases' arithmetic"""
    H, W, Cout = 24, 40, 32
    x0, x1, w, b = R.stem_inputs(H, W, True, Cout, 2, seed=9)
    x = R.stem_planes(x0, x1)
    ref, tol = R.conv7_ref64(x, w, b, 2, True, R.IN_MUL, R.IN_ADD)
    items = np.arange(2 * 12 * 3 * Cout)
    rows, y, t = R.stem_ref64_at(lambda kb, y0, y1, a0, a1: x[kb, :, y0:y1, a0:a1], w, b, H, W, items, True, R.IN_MUL, R.IN_ADD)
    assert len(rows) == ref.size
    assert np.abs(y - ref[tuple(rows.T)]).max() <= 1e-12 and (t >= tol[tuple(rows.T)] * (1 - 1e-12)).all()
    B, H, W, Cout = R.STEM_CAP
    total = B * (H // 2) * ((W // 2 + 7) // 8) * Cout
    assert R.CAP < total <= R.CAP + (1 << 16)
    B, h, w, C = R.GATHER_CAP
    assert B * ((h + 1) // 2) * ((w + 1) // 2) * C // 4 > R.CAP


# ------------------------------------------------------------------------------------------------------------ gather_s2, halve
@pytest.mark.parametrize("h,w,C", R.GH_CASES)
def test_gather_and_halve(h, w, C):
    x = R.gh_input(h, w, C, seed=h * 10 + w)
    assert np.array_equal(R.gather_ref(x), x[:, ::2, ::2].astype(np.float64))
    ref, tol = R.halve_ref64(x)
    got = R.halve_restated(x)
    assert got.dtype == F32 and got.shape == ref.shape == (2, h // 2, w // 2, C)
    assert worst(got, ref, tol) <= 0.5
    # the written-out mean is F.interpolate's
    v = x[:, :2 * (h // 2), :2 * (w // 2)].astype(np.float64)
    assert np.abs(0.25 * (v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]) - ref).max() <= 1e-14
    # a block that starts one column late: outside the bound nearly everywhere (gather: not the same bits)
    if w >= 5:
        late = R.halve_restated(x[:, :, 1:])
        n = min(late.shape[2], got.shape[2])
        assert (np.abs(late[:, :, :n] - ref[:, :, :n]) > tol[:, :, :n]).mean() > 0.99
        assert not np.array_equal(x[:, ::2, 1::2][:, :, :n], x[:, ::2, ::2][:, :, :n])


# ------------------------------------------------------------------------------------------------------------ correlation lookup
LK_CASES = [(h, w, r, levels) for h, w in R.LK_MAPS for r, levels in R.LK_CONFIGS]


@pytest.mark.parametrize("h,w,r,levels", LK_CASES)
def test_lookup_restatement_routes_and_families(h, w, r, levels):
    corr, qx, qy, flow, fam = R.lk_inputs(h, w, r, levels, seed=h * 100 + w + 10 * r + levels)
    win, Q = 2 * r + 1, 2 * h * w
    assert all(hl >= 2 and wl >= 2 for hl, wl in R.lk_levels(h, w, levels))
    ref = R.lookup_ref64(corr, qx, qy, flow, r)
    assert ref.shape == (Q, levels * win * win)
    # two routes to the float64 reference: grid_sample on normalised coordinates, and floor with the four weights
    assert np.abs(ref - R.lookup_ref64(corr, qx, qy, flow, r, route="explicit")).max() <= 1e-12
    tol = R.lookup_tol(corr, qx, qy, flow, r)
    got = R.lookup_restated(corr, qx, qy, flow, r)
    assert worst(got, ref, tol) <= 0.5
    f = {name: fam == k for k, name in enumerate(R.LK_FAMILIES)}
    assert all(v.sum() >= Q // 5 - 1 for v in f.values())
    # whole windows outside: exactly zero, reference and restatement
    assert not ref[f["outside"]].any() and not got[f["outside"]].any()
    # inside: at least 90 % of the bilinear taps of the window centres lie inside the map (the windows themselves reach past a 2 x 2
    # level whatever the target), and the samples there are non-zero
    centre = R.lookup_centre_taps(corr, qx, qy, flow, r)
    assert centre[f["inside"]].mean() >= 0.9
    mid = np.arange(levels) * win * win + r * win + r
    assert (ref[f["inside"]][:, mid] != 0).mean() >= 0.9
    # integral targets: the samples at the window centre ARE taps
    k = f["integral"]
    cx, cy = (qx + flow[:, 0])[k].astype(int), (qy + flow[:, 1])[k].astype(int)
    assert np.array_equal(R.lookup_ref64(corr, qx, qy, flow, r, route="explicit")[k][:, r * win + r], corr[0][k][np.arange(k.sum()), cy, cx].astype(np.float64))
    # border families: windows (one per query and level) holding both zero and non-zero samples, in at least 20 % of them
    for name in ("border", "exact"):
        wv = ref[f[name]].reshape(-1, levels, win * win)
        both = ((wv == 0).any(axis=2) & (wv != 0).any(axis=2)).mean()
        assert both >= 0.2, (name, both)
    # queries are independent: no two share a correlation row
    assert len(np.unique(corr[-1].reshape(Q, -1), axis=0)) == Q


def test_lookup_bound_sees_a_transposed_window_and_a_query_offset():
    h, w, r, levels = 22, 21, 4, 4
    corr, qx, qy, flow, fam = R.lk_inputs(h, w, r, levels, seed=h * 100 + w + 10 * r + levels)
    win = 2 * r + 1
    ref, tol = R.lookup_ref64(corr, qx, qy, flow, r), R.lookup_tol(corr, qx, qy, flow, r)
    got = R.lookup_restated(corr, qx, qy, flow, r)
    live = fam != R.LK_FAMILIES.index("outside")
    # first window index moving y instead of x
    t = got.reshape(-1, levels, win, win).transpose(0, 1, 3, 2).reshape(got.shape)
    off = ~np.eye(win, dtype=bool).reshape(-1)
    bad = (np.abs(t - ref) > tol).reshape(-1, levels, win * win)[live][:, 0, off]
    assert bad.mean() > 0.5
    # the correlation row of the next query
    shifted = R.lookup_restated([np.roll(c, 1, axis=0) for c in corr], qx, qy, flow, r)
    assert (np.abs(shifted - ref) > tol)[live][:, :win * win].mean() > 0.5


def test_lookup_cap_case_is_the_smallest():
    B, h, w, r, levels, ldo = R.LK_CAP
    assert ldo == R.lk_ldos(r, levels)[2] == 352
    assert B * h * w * ldo > R.CAP >= (B - 1) * h * w * ldo


# ------------------------------------------------------------------------------------------------------------ convex up-sampling
@pytest.mark.parametrize("h,w", R.UP_SHAPES)
@pytest.mark.parametrize("family", R.UP_FAMILIES)
def test_upsample_restatement_uses_half_the_bound(h, w, family):
    flow, mask = R.up_inputs(h, w, family, seed=h * 100 + w)
    ref = R.up_ref64(flow, mask)
    assert ref.shape == (2, 2, 8 * h, 8 * w)
    assert np.abs(ref - R.up_ref64(flow, mask, route="explicit")).max() <= 1e-12 * 8 * np.abs(flow).max()
    tol = R.up_tol(flow, mask)
    assert worst(R.up_restated(flow, mask), ref, tol) <= 0.5
    p, _, _ = R._up_parts(flow, mask)
    if family == "onehot":                                   # near one-hot: the largest weight is 1 to fp32 in a quarter of the pixels,
        big = p.max(axis=3)                                  # above 0.99 in half of them, and some exponentials underflow fp32 altogether
        assert (big > 1 - 2.0 ** -24).mean() > 0.25 and np.median(big) > 0.99
        assert (mask.reshape(2, h, w, 9, 64).max(axis=3) - mask.reshape(2, h, w, 9, 64).min(axis=3) > 104).any()
    if family == "border":
        out = R.up_outside(h, w)[None, :, :, :, None]
        cell = out.any(axis=3)[..., 0][0]
        assert cell.all() if min(h, w) <= 2 else (cell.sum() == 2 * h + 2 * w - 4)
        mass = (p * out).sum(axis=3)[:, cell].mean()
        assert mass >= 0.2, mass


def test_upsample_bound_sees_a_softmax_over_the_inside_taps():
    """Renormalising over the taps inside the map changes border cells only, and there it leaves the bound in both the plain and the
    border-heavy family (and is invisible in the interior: the two restatements agree bit for bit there)."""
    h, w = 16, 20
    for family in ("normal", "border"):
        flow, mask = R.up_inputs(h, w, family, seed=h * 100 + w)
        ref, tol = R.up_ref64(flow, mask), R.up_tol(flow, mask)
        wrong = R.up_restated(flow, mask, renormalise_inside=True)
        edge = R.up_border_pixels(h, w)
        bad = np.abs(wrong - ref) > tol
        assert bad[:, :, edge].mean() > 0.95, family
        assert np.array_equal(wrong[:, :, ~edge], R.up_restated(flow, mask)[:, :, ~edge])


# ------------------------------------------------------------------------------------------------------------ the movers
def test_mover_cases_and_a_second_trip_offset():
    rows, ldd, c0, lds, Cs = R.PACK_CAP
    assert rows * Cs > R.CAP and ldd >= c0 + Cs and lds >= Cs
    assert all(ldd >= c0 + Cs and lds >= Cs for _, ldd, c0, lds, Cs in R.PACK_CASES)
    assert R.SCALE_CAP > R.CAP
    # a second trip that starts one element late (i += gridDim.x * 256 + 1) is visible bit for bit: elements differ from their neighbours
    n = 4099
    x = np.random.default_rng(1).standard_normal(n).astype(F32)
    s = F32(1.0 / np.sqrt(256.0))
    right = x * s
    wrong = right.copy()
    cap = 4096                                            # a small stand-in for the cap
    wrong[cap:] = np.append(x[cap + 1:], F32(0)) * s
    assert not np.array_equal(wrong, right)
    dst, src = np.zeros((7, 9), F32), np.arange(35, dtype=F32).reshape(7, 5)
    out = R.pack_restated(dst, 3, src, 4)
    assert np.array_equal(out[:, 3:7], src[:, :4]) and not out[:, :3].any() and not out[:, 7:].any()
    for images, n_per in R.ABSMAX_CASES:
        x = R.absmax_inputs(images, n_per, seed=n_per)
        m = np.abs(x).max(axis=1)
        assert m[0] == F32(3.5) and (n_per == 1 or np.abs(x[0, :-1]).max() < 3.5)
        assert images < 2 or m[1] == F32(7.25)
    assert any(n < 64 * 1024 for _, n in R.ABSMAX_CASES) and any(n > 64 * 1024 for _, n in R.ABSMAX_CASES)
