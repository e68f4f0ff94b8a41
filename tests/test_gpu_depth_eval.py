"""GPU: depth evaluation on the device (csrc/metrics.hip through evaluate_depth(device='cuda'), ops.depth_align, ops.depth_metrics)
against the host path of tool/depth_metrics.py and numpy float64.  Clips and host references: depth_eval_cases.py (five families at
(1,5,7), (3,37,41), (2,96,128), once at (8,288,512) with invalid bands and a frame without a valid pixel).

The LAD result is accepted by its objective value f(s, t) = sum |s p + t - g| (numpy float64 on the valid pixels): the problem is
convex, so a point with a lower f is a better answer whatever scipy's parameters are.  The 1e-9 is the margin over float64 summation
noise.  AbsRel(device) is held to the project's own 1e-4 against AbsRel(host)."""
import functools
import os

import numpy as np
import pytest
import torch

import depth_eval_cases as dc
from conftest import GOLDEN, record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEANS = ("abs_rel", "sq_rel", "rmse", "log_rmse")
ALL_CASES = dc.SMALL_CASES + (dc.LARGE,)
case_id = lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}"


def evaluate(pred, gt, **kw):
    from align3r_amd.tool.depth_metrics import evaluate_depth
    kw.setdefault("depth_max", dc.DEPTH_MAX)
    return evaluate_depth(pred, gt, device=DEV, **kw)


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_lad_objective_and_abs_rel(case):
    pred, gt = dc.make_clip(*case)
    p, g = dc.valid_pairs(pred, gt)
    host = dc.host_lad(*case)
    m = evaluate(pred, gt, mode="lad")
    f_dev = dc.lad_objective(p, g, m["scale"], m["shift"])
    excess, d_abs_rel = (f_dev - host["f"]) / host["f"], abs(m["abs_rel"] - host["metrics"]["abs_rel"])
    record_margin(f"depth_eval_lad[{case_id(case)}]", objective_excess_over_host=excess, abs_rel_diff=d_abs_rel)
    assert m["n_valid"] == p.size
    assert f_dev <= host["f"] * (1 + 1e-9), (excess, m, host)
    assert d_abs_rel <= 1e-4, (d_abs_rel, m, host)


def test_lad_objective_against_reference_goldens():
    z = np.load(os.path.join(GOLDEN, "depth_eval.npz"))
    vals = {}
    for k in range(3):
        pred, gt, (rs, rt) = z[f"pred_{k}"], z[f"gt_{k}"], z[f"st_{k}"]
        p, g = dc.valid_pairs(pred, gt)
        m = evaluate(pred, gt, mode="lad")
        f_dev, f_ref = dc.lad_objective(p, g, m["scale"], m["shift"]), dc.lad_objective(p, g, rs, rt)
        vals[f"excess_{k}"] = (f_dev - f_ref) / f_ref
        vals[f"abs_rel_diff_{k}"] = abs(m["abs_rel"] - dc.metrics_np(p, g, rs, rt)["abs_rel"])
    record_margin("depth_eval_lad_goldens", **vals)
    for k in range(3):
        assert vals[f"excess_{k}"] <= 1e-9, vals
        assert vals[f"abs_rel_diff_{k}"] <= 1e-4, vals


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_metrics_with_injected_scale_shift(case):
    """n_valid equal; the four means within 1e-10 relative of numpy float64 (float64 eps x 1e6 terms, worst case); each delta within
    1 / n_valid (a ratio that sits on a threshold to the last bit)."""
    pred, gt = dc.make_clip(*case)
    host = dc.host_lad(*case)
    want = host["metrics"]
    m = evaluate(pred, gt, scale_shift=(host["s"], host["t"]))
    assert m["n_valid"] == want["n_valid"]
    assert m["scale"] == host["s"] and m["shift"] == host["t"]
    errs = {k: rel(m[k], want[k]) for k in MEANS}
    errs.update({k: abs(m[k] - want[k]) * want["n_valid"] for k in ("d1", "d2", "d3")})
    record_margin(f"depth_eval_metrics[{case_id(case)}]", **errs)
    for k in MEANS:
        assert errs[k] <= 1e-10, (k, errs)
    for k in ("d1", "d2", "d3"):
        assert errs[k] <= 1.0 + 1e-9, (k, errs)


def _rule_against_host(case, mode):
    pred, gt = dc.make_clip(*case)
    p, g = dc.valid_pairs(pred, gt)
    hs, ht = dc.host_rule(p, g, mode)
    m = evaluate(pred, gt, mode=mode)
    errs = dict(scale=rel(m["scale"], hs), shift=rel(m["shift"], ht) if ht != 0.0 else abs(m["shift"]))
    record_margin(f"depth_eval_{mode}[{case_id(case)}]", **errs)
    assert m["n_valid"] == p.size
    assert errs["scale"] <= 1e-9 and errs["shift"] <= 1e-9, (errs, m, hs, ht)
    assert abs(m["abs_rel"] - dc.metrics_np(p, g, hs, ht)["abs_rel"]) <= 1e-8


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_lstsq_rule_matches_host(case):
    """(s, t) within 1e-9 relative of np.linalg.lstsq.  Measured on an MI355X: scale within 4.9e-15, shift within 1.4e-14."""
    _rule_against_host(case, "lstsq")


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_scale_rule_matches_host(case):
    """s within 1e-9 relative of the host's mean ratio + 10 IRLS passes.  The passes amplify a last-bit difference in the first sums
    about 1e12 times (numpy alone moves the host's answer by 1e-3 when the pixels are reordered:
    test_depth_eval_cpu.py::test_host_scale_rule_depends_on_the_summation_order), so the bound can be met only with the host's own
    sums: the device compacts the valid pixels in order and adds with numpy's summation tree (csrc/metrics.hip, 'scale')."""
    _rule_against_host(case, "scale")


def _median_inputs():
    """Odd and even valid counts, duplicated values around the middle, negative predictions, an all-negative pred."""
    pred, gt = (a.copy() for a in dc.make_clip("cauchy", (3, 37, 41)))
    assert (pred[np.isfinite(pred)] < 0).any()
    out = {"cauchy_as_is": (pred, gt)}
    gt2 = gt.copy()
    gt2.reshape(-1)[np.flatnonzero((gt.reshape(-1) > 1.0) & (gt.reshape(-1) < 60.0))[0]] = 0.0       # one valid pixel fewer: the other parity
    out["cauchy_other_parity"] = (pred, gt2)
    out["duplicates"] = (np.round(pred * 2.0) / 2.0, np.round(gt))                                  # hundreds of copies of each value
    out["duplicates_other_parity"] = (np.round(pred * 2.0) / 2.0, np.round(gt2))
    out["all_negative"] = (-np.abs(pred) - 1.0, gt)
    p7, g7 = dc.make_clip("cauchy", (1, 5, 7))
    out["tiny"] = (p7, g7)
    return out


def test_median_rule_order_statistics_are_those_of_np_partition():
    from align3r_amd import ops
    parities = set()
    for name, (pred, gt) in _median_inputs().items():
        with np.errstate(invalid="ignore"):
            valid = (gt > 1e-3) & (gt < dc.DEPTH_MAX)
        p32, g32 = pred[valid], gt[valid]
        m = p32.size
        parities.add(m % 2)
        lo, hi = (m - 1) // 2, m // 2
        want = [np.partition(p32, [lo, hi])[[lo, hi]], np.partition(g32, [lo, hi])[[lo, hi]]]
        st, info = ops.depth_align(up(pred.astype(np.float32)), up(gt.astype(np.float32)), dc.DEPTH_MAX, "median")
        st, info = st.cpu().numpy(), info.cpu().numpy()
        got = info[4:8].astype(np.float32)
        assert np.array_equal(got.astype(np.float64), info[4:8]), name                              # float32 values, stored exactly
        assert got.tobytes() == np.concatenate(want).astype(np.float32).tobytes(), (name, got, want)
        assert info[0] == m
        med_p, med_g = np.median(p32.astype(np.float64)), np.median(g32.astype(np.float64))
        assert info[8] == med_p and info[9] == med_g, name
        assert st[0] == med_g / med_p and st[1] == 0.0, name
        res = evaluate(pred, gt, mode="median")
        assert res["scale"] == st[0] and res["n_valid"] == m
    assert parities == {0, 1}


def test_validity_bounds_are_strict():
    pred, gt = (a.copy() for a in dc.make_clip("lognormal", (3, 37, 41)))
    flat = gt.reshape(-1)
    k = int(np.flatnonzero((flat > 1.0) & (flat < 60.0))[7])
    n_valid = lambda: evaluate(pred, gt, scale_shift=(3.0, 0.0))["n_valid"]
    base = n_valid()
    with np.errstate(invalid="ignore"):
        assert base == int(((gt > 1e-3) & (gt < dc.DEPTH_MAX)).sum())          # the NaN, the inf and the two bounds of the clip: never counted
    lo, hi = np.float32(1e-3), np.float32(dc.DEPTH_MAX)
    for inside, bound in ((np.nextafter(lo, np.float32(1.0)), lo), (np.nextafter(hi, np.float32(1.0)), hi)):
        flat[k] = inside
        assert n_valid() == base
        flat[k] = bound
        assert n_valid() == base - 1
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        flat[k] = bad
        assert n_valid() == base - 1


def _offset_copy(a):
    """The same float32 data in a device buffer that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:]
    view.copy_(torch.from_numpy(np.array(a).reshape(-1)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _two_stride_clip():
    n = 2 * 1024 * 1024 + 100_003                          # more than two grid strides of 1024 workgroups x 1024 elements, n % 4 = 3
    rng = np.random.default_rng(5)
    gt = rng.uniform(0.0005, 80.0, n).astype(np.float32)    # some below 1e-3, some beyond depth_max
    pred = (gt.astype(np.float64) / 2.5 * np.exp(0.05 * rng.standard_normal(n)) + 0.3).astype(np.float32)
    return pred, gt


@pytest.mark.parametrize("which", ["below_one_block", "medium", "two_grid_strides"])
def test_offset_pointers_and_repeatability(which):
    """The scalar path (pointers 4 bytes past a 16-byte boundary, or only one of them) against the 16-byte path to 1e-12; the same call
    twice is bitwise equal (every rule); n below one workgroup, and n of more than two grid strides.  The two paths add in another
    order, so the 1e-12 is asked of what is a fixed function of the sums: the metrics for a given (s, t), 'lstsq', 'median'.  The LAD
    search is iterative and may take another route: there the objectives are compared (1e-9, the bound of the LAD test).  'scale' adds the
    compacted pixels in the host's order whatever the load path: equal bits."""
    if which == "below_one_block":
        pred, gt = dc.make_clip("sqrt", (1, 5, 7))
    elif which == "medium":
        pred, gt = dc.make_clip("bands", (2, 96, 128))
    else:
        pred, gt = _two_stride_clip()
    pred, gt = pred.reshape(-1), gt.reshape(-1)
    p, g = dc.valid_pairs(pred, gt)
    hs, ht = dc.host_rule(p, g, "lstsq")
    a_pred, a_gt = up(pred), up(gt)
    assert a_pred.data_ptr() % 16 == 0 and a_gt.data_ptr() % 16 == 0
    o_pred, o_gt = _offset_copy(pred), _offset_copy(gt)
    worst = 0.0
    for kw in (dict(scale_shift=(hs, ht)), dict(mode="lstsq"), dict(mode="scale"), dict(mode="median"), dict(mode="lad")):
        aligned = evaluate(a_pred, a_gt, **kw)
        assert aligned == evaluate(a_pred, a_gt, **kw), kw                      # bitwise: floats compared with ==
        offset, mixed = evaluate(o_pred, o_gt, **kw), evaluate(o_pred, a_gt, **kw)
        assert offset == evaluate(o_pred, o_gt, **kw), kw
        assert offset["n_valid"] == mixed["n_valid"] == aligned["n_valid"] == p.size
        if kw.get("mode") == "lad":
            f = [dc.lad_objective(p, g, r["scale"], r["shift"]) for r in (aligned, offset, mixed)]
            assert max(f) <= min(f) * (1 + 1e-9), f
            continue
        if kw.get("mode") == "scale":
            assert offset["scale"] == aligned["scale"] == mixed["scale"]
        for other in (offset, mixed):
            for k in MEANS + ("scale", "shift"):
                e = abs(other[k] - aligned[k]) / max(abs(aligned[k]), 1e-300)
                worst = max(worst, e)
                assert e <= 1e-12, (kw, k, other[k], aligned[k])
    want = dc.metrics_np(p, g, hs, ht)
    got = evaluate(o_pred, o_gt, scale_shift=(hs, ht))
    assert got["n_valid"] == want["n_valid"]
    for k in MEANS:
        assert rel(got[k], want[k]) <= 1e-10, (k, got[k], want[k])
    for a, b in ((a_pred, a_gt), (o_pred, o_gt)):
        got = evaluate(a, b, mode="lstsq")
        assert rel(got["scale"], hs) <= 1e-9 and rel(got["shift"], ht) <= 1e-9
    record_margin(f"depth_eval_offset[{which}]", worst_rel_diff_offset_vs_aligned=worst)


def test_refusals_and_the_call_after():
    pred, gt = dc.make_clip("lognormal", (3, 37, 41))
    good = evaluate(pred, gt, mode="lstsq")
    for bad_gt in (np.zeros_like(gt), np.full_like(gt, np.nan), np.full_like(gt, 2 * dc.DEPTH_MAX)):
        for kw in (dict(mode="lad"), dict(mode="lstsq"), dict(mode="scale"), dict(mode="median"), dict(scale_shift=(1.0, 0.0))):
            with pytest.raises(ValueError, match="no valid pixel"):
                evaluate(pred, bad_gt, **kw)
    one = np.zeros_like(gt)
    one[0, 0, 0] = 5.0                                                          # a single valid pixel fixes no scale and shift
    with pytest.raises(ValueError, match="no valid pixel"):
        evaluate(pred, one, mode="lad")
    with pytest.raises(ValueError, match="shape"):
        evaluate(pred, gt[:, :-1], mode="lad")
    with pytest.raises(ValueError, match="shape"):
        evaluate(up(pred), up(gt).reshape(-1), mode="lad")
    with pytest.raises(ValueError, match="bad alignment"):
        evaluate(pred, gt, mode="huber")
    assert evaluate(pred, gt, mode="lstsq") == good


def test_input_forms_agree():
    pred, gt = dc.make_clip("bands", (3, 37, 41))
    for kw in (dict(mode="lad"), dict(mode="lstsq")):
        base = evaluate(pred, gt, **kw)
        assert list(base) == ["abs_rel", "sq_rel", "rmse", "log_rmse", "d1", "d2", "d3", "n_valid", "scale", "shift"]
        forms = dict(device_tensors=(up(pred), up(gt)), host_tensors=(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy())),
                     float64_arrays=(pred.astype(np.float64), gt.astype(np.float64)), list_of_arrays=(list(pred), list(gt)),
                     list_of_device_maps=([up(m) for m in pred], [up(m) for m in gt]), mixed=(up(pred), gt))
        for name, (a, b) in forms.items():
            assert evaluate(a, b, **kw) == base, (name, kw)
