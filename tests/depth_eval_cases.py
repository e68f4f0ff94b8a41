"""Shared inputs of the depth-evaluation tests (test_gpu_depth_eval.py, test_depth_eval_cpu.py, golden/make_goldens_depth_eval.py):
synthetic clips of five families, the host references (computed once per case and cached), numpy float64 restatements of the sums.

Families (pred as a function of gt, gt uniform in [0.5, 60)):
  lognormal   pred = gt / 3 * exp(0.1 N(0,1))                       multiplicative noise
  scale100    pred = (gt + 400) / 100 + 0.005 N(0,1)                a 100x scale and a shift of -400: outside the LAD start region
  cauchy      pred = 0.5 gt + 1 + 0.3 Cauchy                        heavy tails, negative predictions
  sqrt        pred = sqrt(gt) + 0.05 N(0,1)                         a distortion no (s, t) removes
  bands       lognormal with invalid regions: rows of gt = 0, columns beyond depth_max, (in the large clip) a frame without a valid pixel
Every clip's gt also holds one value exactly float32(1e-3), one exactly depth_max, one NaN and one inf (all invalid); pred is NaN at
the NaN gt only.

Seeds.  The LAD tests bound AbsRel(device) against AbsRel(host), and the host's scipy BFGS on this non-smooth objective "stops where
it stops": on some draws (most 35-pixel ones) it ends with an objective 1e-5 .. 1e-2 above the minimum and an AbsRel that is off by
more than the 1e-4 the comparison allows, whatever the device computes.  The comparison says something only where the host reached
the minimum, so a case takes the first draw k = 0, 1, 2, ... (SEED_OFFSET) at which the host's AbsRel is within 1e-6 of the AbsRel at
the exact LAD minimum; test_depth_eval_cpu.py checks that against a linear-programming solution for the draws that were skipped to.
The objective assertion f(device) <= f(host) (1 + 1e-9) does not depend on this choice."""
import functools

import numpy as np

DEPTH_MAX = 70.0
FAMILIES = ("lognormal", "scale100", "cauchy", "sqrt", "bands")
SHAPES = ((1, 5, 7), (3, 37, 41), (2, 96, 128))
LARGE = ("bands", (8, 288, 512))
SEED_OFFSET = {("lognormal", (1, 5, 7)): 1, ("scale100", (1, 5, 7)): 54, ("cauchy", (1, 5, 7)): 1, ("sqrt", (1, 5, 7)): 38, ("bands", (1, 5, 7)): 10,
               ("cauchy", (2, 96, 128)): 1}
SMALL_CASES = tuple((f, s) for s in SHAPES for f in FAMILIES)


@functools.lru_cache(maxsize=None)
def make_clip(family, shape):
    """-> pred, gt float32 [T, H, W] (read-only: shared between tests)."""
    T, H, W = shape
    n = T * H * W
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + n + 100000 * SEED_OFFSET.get((family, shape), 0))
    gt = rng.uniform(0.5, 60.0, n).astype(np.float32)
    g = gt.astype(np.float64)
    if family in ("lognormal", "bands"):
        pred = g / 3.0 * np.exp(0.1 * rng.standard_normal(n))
    elif family == "scale100":
        pred = (g + 400.0) / 100.0 + 0.005 * rng.standard_normal(n)
    elif family == "cauchy":
        pred = 0.5 * g + 1.0 + 0.3 * rng.standard_cauchy(n)
    else:
        pred = np.sqrt(g) + 0.05 * rng.standard_normal(n)
    pred = pred.astype(np.float32).reshape(shape)
    gt = gt.reshape(shape)
    if family == "bands":
        gt[:, H // 3:H // 3 + max(H // 8, 1), :] = 0.0                    # a band without ground truth
        gt[:, :, W - max(W // 10, 1):] = 2.0 * DEPTH_MAX                  # a band beyond depth_max
        if T >= 8:
            gt[5] = 0.0                                                   # a frame without a valid pixel
    flat_g, flat_p = gt.reshape(-1), pred.reshape(-1)
    k = rng.choice(n, 4, replace=False)
    flat_g[k[0]] = np.float32(1e-3)
    flat_g[k[1]] = np.float32(DEPTH_MAX)
    flat_g[k[2]] = np.nan
    flat_g[k[3]] = np.inf
    flat_p[k[2]] = np.nan
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def valid_pairs(pred, gt, depth_max=DEPTH_MAX):
    """The host's selection (evaluate_depth): float64 copies of the pixels with 1e-3 < gt < depth_max."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    with np.errstate(invalid="ignore"):
        valid = np.logical_and(gt > 1e-3, gt < depth_max)
    return pred[valid].astype(np.float64), gt[valid].astype(np.float64)


def lad_objective(p, g, s, t):
    """f(s, t) = sum |s p + t - g| in float64 over the valid pixels."""
    return float(np.sum(np.abs(s * p + t - g)))


def metrics_np(p, g, s, t, depth_max=DEPTH_MAX):
    """The sums of evaluate_depth for a given (s, t), numpy float64 on the valid pixels (the same expressions as the host path)."""
    aligned = np.clip(s * p + t, 1e-5, depth_max)
    ratio = np.maximum(aligned / g, g / aligned)
    return dict(abs_rel=float(np.mean(np.abs(aligned - g) / g)), sq_rel=float(np.mean((aligned - g) ** 2 / g)),
                rmse=float(np.sqrt(np.mean((aligned - g) ** 2))), log_rmse=float(np.sqrt(np.mean((np.log(aligned) - np.log(g)) ** 2))),
                d1=float(np.mean(ratio < 1.25)), d2=float(np.mean(ratio < 1.25 ** 2)), d3=float(np.mean(ratio < 1.25 ** 3)), n_valid=int(p.size))


@functools.lru_cache(maxsize=None)
def host_lad(family, shape):
    """The host path's LAD (s, t) of a case (scipy's minimize started at the median ratio, as evaluate_depth(mode='lad') runs it), its
    objective value and the metrics at that point."""
    from align3r_amd.tool.depth_metrics import _lad_scale_shift
    p, g = valid_pairs(*make_clip(family, shape))
    s, t = _lad_scale_shift(p, g, np.median(g) / np.median(p))
    return dict(s=s, t=t, f=lad_objective(p, g, s, t), metrics=metrics_np(p, g, s, t))


def lad_exact(p, g):
    """The exact LAD minimum by linear programming (min sum e, -e <= s p + t - g <= e): (s, t).  For small clips."""
    from scipy.optimize import linprog
    n = p.size
    c = np.concatenate([[0.0, 0.0], np.ones(n)])
    A = np.block([[p[:, None], np.ones((n, 1)), -np.eye(n)], [-p[:, None], -np.ones((n, 1)), -np.eye(n)]])
    res = linprog(c, A_ub=A, b_ub=np.concatenate([g, -g]), bounds=[(None, None)] * 2 + [(0, None)] * n, method="highs")
    assert res.status == 0, res.message
    return float(res.x[0]), float(res.x[1])


def host_rule(p, g, mode):
    """(s, t) of the host's 'lstsq', 'scale' and 'median' rules (the expressions of align_depth)."""
    if mode == "lstsq":
        (s, t), *_ = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), g, rcond=None)
        return float(s), float(t)
    if mode == "scale":
        s = np.nanmean(g) / np.nanmean(p)
        for _ in range(10):
            w = 1.0 / (np.abs(s * p - g) + 1e-8)
            s = np.sum(w * p * g) / np.sum(w * p ** 2)
        return float(max(s, 1e-3)), 0.0
    if mode == "median":
        return float(np.median(g) / np.median(p)), 0.0
    raise ValueError(mode)
