"""CPU: the fp32 arithmetic of the producer kernels (csrc/elementwise.hip), restated in numpy in the kernels' own order, stays inside
every tolerance that tests/test_gpu_producers_f64.py asserts -- for every family, width and shape that test uses.  So a failure of
the GPU test means a kernel computes something else, not that fp32 in that order cannot meet the bound.  Also: the tolerances are
tight enough to see the faults they are there for (a variance over D - 1, swapped weights of the interpolation)."""
import numpy as np
import pytest
import torch

import producer_refs as R
from test_gpu_up2x_forms import SHAPES as UP_FORM_SHAPES

LN_WIDTHS = sorted({D for _, D in R.LN_F32_CASES} | set(R.LN_FH2_D) | {R.LN_FH2_UNALIGNED_D, R.LN_FH2_PERSISTENT[1]})
UP_SHAPES = list(dict.fromkeys(UP_FORM_SHAPES + R.UP_EXTRA + R.UP_BF3))


def _orders(D):
    return [o for o, per in (("strided", 1), ("f4", 4), ("f8", 8)) if D % per == 0]


@pytest.mark.parametrize("D", LN_WIDTHS)
def test_layernorm_lane_orders_stay_inside_the_tolerance(D):
    x, w, b, fam = R.ln_inputs(80, D, seed=1000 + D)
    assert len(np.unique(fam)) == len(R.FAMILIES)
    tol, ref = R.ln_tolerances(x, w, b, fam)
    for order in _orders(D):
        y = R.ln_restated(x, w, b, order)
        err = R.ln_family_errors(y, ref, fam)
        for f, e in err.items():
            assert e <= tol[f], (D, order, R.FAMILIES[f], e, tol[f])
        const = fam == R.FAMILIES.index("const")
        assert np.array_equal(y[const], np.broadcast_to(b, y[const].shape)), (D, order)     # mean exact, centred row exactly zero


def test_layernorm_tolerance_sees_a_variance_over_d_minus_1():
    """A sample variance in place of the population variance, at the width where it is smallest (relative 1 / (2 D) = 2.4e-4 at D = 2048)."""
    D = 2048
    x, w, b, fam = R.ln_inputs(80, D, seed=1000 + D)
    tol, ref = R.ln_tolerances(x, w, b, fam)
    x64 = x.astype(np.float64)
    c = x64 - x64.mean(1, keepdims=True)
    wrong = c / np.sqrt((c * c).sum(1, keepdims=True) / (D - 1) + R.LN_EPS) * w + b
    err = R.ln_family_errors(wrong, ref, fam)
    for name in ("plain", "offset", "spike"):
        f = R.FAMILIES.index(name)
        assert err[f] > tol[f], (name, err[f], tol[f])


def test_layernorm_rows_are_distinct():
    x, _, _, fam = R.ln_inputs(83, 64, seed=5)
    keep = fam != R.FAMILIES.index("const")
    assert len(np.unique(x[keep], axis=0)) == int(keep.sum())
    assert len(R.ln_families(15)) == 15 and not R.ln_families(15).any()


@pytest.mark.parametrize("B,H,W,C,crop", UP_SHAPES)
def test_bilinear_restatement_stays_inside_the_bound(B, H, W, C, crop):
    x = R.up_input(B, H, W, C, seed=H * 100 + W)
    ref = R.up_ref64(x, crop)
    got = R.up_restated(x, crop)
    assert got.shape == ref.shape
    tol = R.up_tolerance(x)
    assert (np.abs(got.astype(np.float64) - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    if H > 1 and W > 1:                                     # the written-out formula (used for H = 1, W = 1) is F.interpolate's
        assert np.abs(R.up_formula64(x, crop) - ref).max() <= 1e-12 * np.abs(x).max()


def test_bilinear_bound_sees_swapped_weights():
    x = R.up_input(2, 3, 5, 8, seed=305)
    tol = R.up_tolerance(x)
    x64 = x.astype(np.float64)
    y0, y1, ly = R._up_axis64(3)
    ly = ly[None, :, None, None]
    straight = x64[:, y0] * (1 - ly) + x64[:, y1] * ly                  # one axis is enough
    swapped = x64[:, y0] * ly + x64[:, y1] * (1 - ly)
    assert np.abs(swapped - straight).max() > 1e3 * float(tol.max())


@pytest.mark.parametrize("P,C", R.HEAD_CASES)
def test_head_restatement_stays_inside_the_tolerance(P, C):
    x, w, bias = R.head_inputs(P, C, seed=P + C)
    for bvec in (bias, torch.zeros(4)):
        p64, c64, tol_p, tol_c, dmax, f3max = R.head_refs(x, w, bvec)
        assert dmax < 6 and f3max < 6, (dmax, f3max)
        pts, conf = R.head_restated(x, w, bvec)
        assert np.abs(pts.astype(np.float64) - p64.numpy()).max() <= tol_p
        assert np.abs(conf.astype(np.float64) - c64.numpy()).max() <= tol_c


@pytest.mark.parametrize("B,N,H,D,pmax", [c for c in R.ROPE_CASES if c[1] < 1000] + [(1, 300, 2, 128, 63)])
def test_rope_restatement_stays_inside_the_bound(B, N, H, D, pmax):
    """(the 4 x 4100 x 16 x 128 case is there for its size; its arithmetic is D = 128, pmax = 63 -- restated here on 300 tokens)"""
    tok, pos = R.rope_inputs(B, N, H, D, pmax, seed=D + pmax)
    assert int(pos.max()) == pmax and int(pos.min()) >= 0
    tol = R.rope_tolerance(tok, pmax).numpy()
    for fwd in (1.0, -1.0):
        ref = R.rope_ref64(tok, pos, fwd).numpy()
        got, ang = R.rope_restated(tok, pos, fwd)
        assert (np.abs(got.astype(np.float64) - ref) <= tol).all(), float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())
        q = np.arange(D // 4, dtype=np.float64)
        ang64 = fwd * pos.numpy().astype(np.float64)[:, :, None, :, None] / R.ROPE_BASE ** (q / (D // 4))
        assert np.abs(ang - ang64).max() <= pmax * 2.0 ** -23
    back = R.rope_ref64(R.rope_ref64(tok, pos, 1.0), pos, -1.0).numpy()
    assert np.abs(back - tok.double().numpy()).max() < 1e-12
