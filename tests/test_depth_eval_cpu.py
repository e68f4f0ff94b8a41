"""CPU (no GPU): the depth-evaluation entry points (csrc/metrics.hip: a3r_depth_eval_workspace_bytes, a3r_depth_align,
a3r_depth_metrics) refuse bad arguments before they touch the device; evaluate_depth(device='cuda') has no CPU fallback and without
`device` is the host path with the keys it always had; average_depth_metrics against a hand computation; the clips whose seeds were
skipped to (depth_eval_cases.SEED_OFFSET) against an exact LAD solution."""
import ctypes as C

import numpy as np
import pytest

import depth_eval_cases as dc


def test_workspace_bytes():
    from align3r_amd import _lib
    lib = _lib.load()
    for n in (1, 35, 1 << 20, (1 << 31) - 1):
        assert lib.a3r_depth_eval_workspace_bytes(n) > 0
    assert lib.a3r_depth_eval_workspace_bytes(0) == 0 and lib.a3r_depth_eval_workspace_bytes(-5) == 0


def test_refusals_name_the_argument():
    """Every refusal comes before anything is launched: fake (never dereferenced) pointers do."""
    from align3r_amd import _lib
    lib = _lib.load()
    n = 1000
    need = int(lib.a3r_depth_eval_workspace_bytes(n))
    fake = C.c_void_p(1 << 20)

    def align(pred=fake, gt=fake, n=n, depth_max=70.0, mode=0, ws=fake, ws_bytes=need, st=fake, info=fake):
        rc = lib.a3r_depth_align(pred, gt, n, depth_max, mode, ws, ws_bytes, st, info, None)
        return rc, lib.a3r_last_error().decode()

    def metrics(pred=fake, gt=fake, n=n, depth_max=70.0, st=fake, ws=fake, ws_bytes=need, out=fake):
        rc = lib.a3r_depth_metrics(pred, gt, n, depth_max, st, ws, ws_bytes, out, None)
        return rc, lib.a3r_last_error().decode()

    for call, who in ((align, "a3r_depth_align"), (metrics, "a3r_depth_metrics")):
        for kw, word in ((dict(pred=None), "null pred"), (dict(gt=None), "null gt"), (dict(n=0), "n = 0"), (dict(n=-3), "n = -3"),
                         (dict(n=1 << 31), "too large"), (dict(depth_max=1e-3), "depth_max"), (dict(depth_max=float("nan")), "depth_max"),
                         (dict(ws=None), "null workspace"), (dict(ws_bytes=need - 1), "workspace_bytes too small"),
                         (dict(ws=C.c_void_p((1 << 20) + 8)), "16-byte aligned"), (dict(st=None), "null st_dev")):
            rc, msg = call(**kw)
            assert rc != 0 and who in msg and word in msg, (who, kw, rc, msg)
    for kw, word in ((dict(mode=4), "unknown mode 4"), (dict(mode=-1), "unknown mode -1"), (dict(info=None), "null info_dev")):
        rc, msg = align(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc, msg = metrics(out=None)
    assert rc != 0 and "null out_dev" in msg
    with pytest.raises(RuntimeError, match="workspace_bytes too small"):
        _lib.check(lib.a3r_depth_metrics(fake, fake, n, 70.0, fake, fake, 16, fake, None))


def test_device_path_has_no_cpu_fallback():
    import torch
    from align3r_amd import ops
    from align3r_amd.tool.depth_metrics import evaluate_depth
    pred, gt = dc.make_clip("lognormal", (1, 5, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_depth(pred, gt, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evaluate_depth(pred, gt, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.depth_align(torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.depth_metrics(torch.zeros(4), torch.zeros(4), 70.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="bad alignment"):
        ops.depth_align(torch.zeros(4), torch.zeros(4), mode="huber")


def test_host_path_is_unchanged():
    """Without `device` the result is the host computation with exactly the keys it always had; scale_shift belongs to the device path."""
    from align3r_amd.tool.depth_metrics import evaluate_depth
    pred, gt = dc.make_clip("bands", (3, 37, 41))
    p, g = dc.valid_pairs(pred, gt)
    for mode in ("lstsq", "scale", "median"):
        m = evaluate_depth(pred, gt, depth_max=dc.DEPTH_MAX, mode=mode)
        assert list(m) == ["abs_rel", "sq_rel", "rmse", "log_rmse", "d1", "d2", "d3", "n_valid"]
        assert m == dc.metrics_np(p, g, *dc.host_rule(p, g, mode))              # the restatement the GPU tests compare with
    m = evaluate_depth(pred, gt, depth_max=dc.DEPTH_MAX, mode="lad")
    assert list(m) == ["abs_rel", "sq_rel", "rmse", "log_rmse", "d1", "d2", "d3", "n_valid"]
    assert m == dc.host_lad("bands", (3, 37, 41))["metrics"]
    assert m == evaluate_depth(pred, gt, depth_max=dc.DEPTH_MAX, mode="lad", device=None)
    with pytest.raises(ValueError, match="scale_shift"):
        evaluate_depth(pred, gt, scale_shift=(1.0, 0.0))


def test_average_depth_metrics_by_hand():
    from align3r_amd.tool.depth_metrics import average_depth_metrics
    a = dict(abs_rel=0.1, sq_rel=0.2, rmse=1.0, log_rmse=0.5, d1=0.9, d2=0.95, d3=1.0, n_valid=100, scale=2.0, shift=0.1)
    b = dict(abs_rel=0.3, sq_rel=0.6, rmse=3.0, log_rmse=0.1, d1=0.5, d2=0.75, d3=0.8, n_valid=300)
    m = average_depth_metrics([a, b])
    assert list(m) == ["abs_rel", "sq_rel", "rmse", "log_rmse", "d1", "d2", "d3", "n_valid"]
    want = dict(abs_rel=(0.1 * 100 + 0.3 * 300) / 400, sq_rel=(0.2 * 100 + 0.6 * 300) / 400, rmse=(1.0 * 100 + 3.0 * 300) / 400,
                log_rmse=(0.5 * 100 + 0.1 * 300) / 400, d1=(0.9 * 100 + 0.5 * 300) / 400, d2=(0.95 * 100 + 0.75 * 300) / 400,
                d3=(1.0 * 100 + 0.8 * 300) / 400)
    for k, v in want.items():
        assert m[k] == pytest.approx(v, rel=1e-15), k
    assert m["n_valid"] == 400
    assert average_depth_metrics([a]) == {k: a[k] for k in m}
    with pytest.raises(ValueError, match="no valid pixel"):
        average_depth_metrics([])


def test_clip_contents():
    """What the GPU tests rely on: the special gt values are there and invalid, pred is NaN only where gt is invalid, the large clip
    has a frame without a valid pixel."""
    for fam, shape in dc.SMALL_CASES + (dc.LARGE,):
        pred, gt = dc.make_clip(fam, shape)
        assert pred.dtype == gt.dtype == np.float32 and pred.shape == gt.shape == shape
        with np.errstate(invalid="ignore"):
            valid = (gt > 1e-3) & (gt < dc.DEPTH_MAX)
        for special in (np.float32(1e-3), np.float32(dc.DEPTH_MAX), np.float32(np.inf)):
            assert (gt == special).sum() >= 1 and not valid[gt == special].any()
        assert np.isnan(gt).sum() == 1 and np.isnan(pred).sum() == 1 and not valid[np.isnan(pred)].any()
        assert valid.sum() >= 20
    pred, gt = dc.make_clip(*dc.LARGE)
    with np.errstate(invalid="ignore"):
        per_frame = ((gt > 1e-3) & (gt < dc.DEPTH_MAX)).reshape(gt.shape[0], -1).sum(1)
    assert per_frame[5] == 0 and (np.delete(per_frame, 5) > 0).all()


@pytest.mark.parametrize("case", [c for c in dc.SEED_OFFSET if c[1] == (1, 5, 7)], ids=lambda c: c[0])
def test_host_reaches_the_lad_minimum_on_the_chosen_draws(case):
    """The rule behind SEED_OFFSET, against an exact solution: on the chosen draw the host's AbsRel is within 1e-6 of the AbsRel at the
    LAD minimum, and the host's objective is not below it."""
    p, g = dc.valid_pairs(*dc.make_clip(*case))
    s, t = dc.lad_exact(p, g)
    h = dc.host_lad(*case)
    assert dc.lad_objective(p, g, s, t) <= h["f"] * (1 + 1e-12)
    assert abs(dc.metrics_np(p, g, s, t)["abs_rel"] - h["metrics"]["abs_rel"]) <= 1e-6


@pytest.mark.parametrize("case", [("cauchy", (3, 37, 41)), ("sqrt", (2, 96, 128)), ("bands", (8, 288, 512))], ids=lambda c: c[0])
def test_host_scale_rule_depends_on_the_summation_order(case):
    """The host's 'scale' rule (mean ratio + 10 IRLS passes with weights 1 / (|s p - g| + 1e-8)) on the same pixels in another order:
    numpy alone moves the answer by far more than the 1e-9 the device is compared with (test_gpu_depth_eval.py::
    test_scale_rule_matches_host), because the passes amplify the last bit of the first sums.  'lstsq' on the same input does not."""
    p, g = dc.valid_pairs(*dc.make_clip(*case))
    perm = np.random.default_rng(0).permutation(p.size)
    s, _ = dc.host_rule(p, g, "scale")
    s_perm, _ = dc.host_rule(p[perm], g[perm], "scale")
    assert abs(s_perm - s) / s > 1e-7
    (a, b), (a_perm, b_perm) = dc.host_rule(p, g, "lstsq"), dc.host_rule(p[perm], g[perm], "lstsq")
    assert abs(a_perm - a) <= 1e-12 * abs(a) and abs(b_perm - b) <= 1e-12 * abs(b)


def test_run_clip_metrics_device_flag():
    from align3r_amd.tool.run_clip import parse
    base = ["--images", "frames", "--weights", "w.pth", "--out", "out"]
    assert parse(base).metrics_device is False and parse(base + ["--gt-depth", "gt"]).metrics_device is False      # the host path stays the default
    assert parse(base + ["--gt-depth", "gt", "--metrics-device"]).metrics_device is True
    with pytest.raises(SystemExit):
        parse(base + ["--metrics-device"])
