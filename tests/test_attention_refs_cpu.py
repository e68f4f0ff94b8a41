"""CPU: the host side of the attention pins (tests/attention_refs.py) at every (family, shape) that tests/test_gpu_attention_f64.py
launches.
  * every family meets the condition that makes it reach what it is there for (the running maximum of `ramp` rises at every
    32-key block, the peak key of `peak*` holds 15 .. 85 % of the mass, |score| >= 30 for `high` / `low`, `ties` is exactly flat);
  * fp32 arithmetic in the kernels' order (the numpy restatements) stays inside the tolerance WITHOUT its factor 4, so a failure
    of the GPU test means that a kernel computes something else;
  * the tolerance can fail: five restatements, each wrong in one place, exceed it (factor 4 included) on the families named."""
import numpy as np
import pytest

import attention_refs as R

ONES = (1.0, 1.0, 1.0, 1.0)
SCALED_MUL, SCALED = (2.0 ** -6, 2.0 ** -6, 2.0 ** -10), (2.0 ** 6, 2.0 ** 6, 2.0 ** 10, 2.0 ** 10)


def test_shape_lists_are_consistent():
    for s in R.SINGLE_PASS_SHAPES + R.LAYOUT_SHAPES + [R.GROUP_SHAPE]:
        assert s in R.SHAPES
    assert R.LAUNCH_B * R.LAUNCH_H == len(R.FAMILIES) > 8
    for i in range(len(R.SHAPES)):                                       # every launch holds every family once
        assert sorted(R.launch_groups(i)) == sorted(R.FAMILIES)
    assert [b * h for b, h in R.GROUP_COUNTS] == [1, 7, 8, 9, 17]


@pytest.mark.parametrize("Nq,Nk", R.SHAPES)
def test_families_meet_their_conditions(Nq, Nk):
    for fam in R.FAMILIES:
        c = R.attn_case(fam, Nq, Nk)
        assert c.q.shape == (Nq, 64) and c.k.shape == c.v.shape == (Nk, 64) and c.q.dtype == np.float32
        assert np.isfinite(c.ref).all() and (c.R > 0).all()
        R.check_family_conditions(fam, c)
    assert np.array_equal(R.attn_case("ties", Nq, Nk).k, np.repeat(R.attn_case("ties", Nq, Nk).k[:1], Nk, 0))
    assert R.attn_case("voff", Nq, Nk).v.min() > 90


@pytest.mark.parametrize("Nq,Nk", R.SHAPES)
def test_restatements_stay_inside_the_bound(Nq, Nk):
    """error <= max(e32, 2^-22 (1 + A_i)) R_i + floor for the fh2 order, and without the floor for the plain fp32 order in 32-key
    (attn_bf3_kernel) and 64-key (attn_kernel) softmax steps"""
    for fam in R.FAMILIES:
        c = R.attn_case(fam, Nq, Nk)
        e = c.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, ONES)) / c.bound(1.0, 1.0)
        assert e.max() <= 1.0, ("fh2", fam, float(e.max()))
        for block in (32, 64):
            e = c.row_errors(R.attn_restate_f32(c.q, c.k, c.v, block)) / c.bound()
            assert e.max() <= 1.0, ("f32", block, fam, float(e.max()))


@pytest.mark.parametrize("Nq,Nk", R.LAYOUT_SHAPES)
def test_scaled_restatement_stays_inside_the_bound(Nq, Nk):
    """q, k x 2^-6 stored at 2^6 and v x 2^-10 stored and written at 2^10: the same bound, which carries the scales; stored at
    scale 1 instead the same inputs pass only through the 2^-25 floor (the second planes are subnormal)."""
    through_floor = 0
    for fam in R.FAMILIES:
        c = R.attn_case(fam, Nq, Nk, SCALED_MUL)
        e = c.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, SCALED))
        assert (e <= c.bound(SCALED[2], SCALED[3])).all(), (fam, float((e / c.bound(SCALED[2], SCALED[3])).max()))
        e1 = c.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, ONES))
        assert (e1 <= c.bound(1.0, 1.0)).all(), (fam, float((e1 / c.bound(1.0, 1.0)).max()))
        through_floor += int((e1 > c.tol()).any())
    assert through_floor >= 5, through_floor


@pytest.mark.parametrize("Nq,Nk", R.SINGLE_PASS_SHAPES)
def test_single_pass_restatement_stays_inside_its_bound(Nq, Nk):
    """truth on the first planes; P rounded once to fp16: 2^-12 R_i on top of the bound"""
    for fam in R.FAMILIES:
        c = R.attn_case(fam, Nq, Nk, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
        e = c.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, ONES, passes=1))
        lim = R.U12 * c.R + c.bound(1.0, 1.0)
        assert (e <= lim).all(), (fam, float((e / lim).max()))
        assert (lim < c.tol(1.0, 1.0)).all()
        full = R.attn_case(fam, Nq, Nk)
        if fam not in ("ties", "voff"):      # (a flat softmax hides the score error; v + 100 is 100 + noise whatever p is)
            assert (full.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, ONES, passes=1)) > full.tol(1.0, 1.0)).any(), fam


# fault -> the families that must see it (at every shape below; (33, 33) has its last key alone in the second block)
MUST_SEE = {
    "no_rescale": ("ramp", "peaklast"),
    "mask_over": ("peaklast", "ties", "low"),
    "mask_under": ("peaklast", "ties", "low"),
    "no_cross": ("sharp", "high", "low", "plain"),
    "no_p1": ("plain", "voff", "ramp"),
}


@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("Nq,Nk", [(33, 33), (33, 97), (129, 130)])
def test_the_tolerance_sees_a_restatement_wrong_in_one_place(Nq, Nk, fault):
    for fam in MUST_SEE[fault]:
        c = R.attn_case(fam, Nq, Nk)
        ratio = c.row_errors(R.attn_restate_fh2(c.q, c.k, c.v, ONES, fault=fault)) / c.tol(1.0, 1.0)
        assert ratio.max() > 1.0, (fault, fam, float(ratio.max()))


def test_max_found_early_needs_no_rescale():
    """peak0 is the family of the alpha == 1 path: leaving the rescale out changes nothing there, which is why `ramp` and the later
    peaks exist"""
    c = R.attn_case("peak0", 129, 130)
    assert np.array_equal(R.attn_restate_fh2(c.q, c.k, c.v, ONES, fault="no_rescale"), R.attn_restate_fh2(c.q, c.k, c.v, ONES))
