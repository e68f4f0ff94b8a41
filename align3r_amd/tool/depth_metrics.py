"""Video-depth accuracy metrics of the reference's evaluation (SURVEY.md 8d "Accuracy metric"; tool/depth_test.py:689-835).

`evaluate_depth(pred, gt, ...)`: valid mask 1e-3 < gt < depth_max (:695-698), ONE scale/shift (or scale) for the whole clip by
the chosen rule (:706-764), clip to [1e-5, depth_max] (:766), then AbsRel / SqRel / RMSE / logRMSE / delta thresholds
(:798-812).  Rules: 'lstsq' (least squares scale + shift), 'lad' (least absolute deviations scale + shift through
scipy.optimize.minimize started at the median ratio: the mode behind the reference's published AbsRel), 'scale' (Weiszfeld
IRLS scale only), 'median' (default: median ratio).
This is the check the north star asks for ("aligned-depth AbsRel within 1e-4 of reference").  Two paths: host numpy + scipy (the
default, `device=None`), and `device='cuda'`: the same rules and sums as HIP kernels (csrc/metrics.hip: streaming float64 reductions,
a radix select for the medians, the LAD minimum by an ellipsoid method driven on the device), opt-in, no CPU fallback.
`average_depth_metrics` is the n_valid-weighted average over sequences (:827-834).
"""
from __future__ import annotations

import numpy as np


def _lad_scale_shift(pred, gt, s0):
    from scipy.optimize import minimize
    res = minimize(lambda p: np.sum(np.abs(p[0] * pred + p[1] - gt)), [s0, 0.0])      # absolute_value_scaling, :689-703
    return float(res.x[0]), float(res.x[1])


def align_depth(pred, gt, mode='lad'):
    """pred, gt: flat float arrays of the valid pixels -> aligned pred (before clipping)."""
    pred = np.asarray(pred, np.float64).reshape(-1)
    gt = np.asarray(gt, np.float64).reshape(-1)
    if mode == 'lstsq':
        A = np.stack([pred, np.ones_like(pred)], 1)
        (s, t), *_ = np.linalg.lstsq(A, gt, rcond=None)
        return s * pred + t
    if mode == 'lad':
        s, t = _lad_scale_shift(pred, gt, np.median(gt) / np.median(pred))
        return s * pred + t
    if mode == 'scale':
        s = np.nanmean(gt) / np.nanmean(pred)
        for _ in range(10):
            w = 1.0 / (np.abs(s * pred - gt) + 1e-8)
            s = np.sum(w * pred * gt) / np.sum(w * pred ** 2)
        return max(s, 1e-3) * pred
    if mode == 'median':
        return pred * (np.median(gt) / np.median(pred))
    raise ValueError(f'bad alignment {mode=}')


METRIC_KEYS = ('abs_rel', 'sq_rel', 'rmse', 'log_rmse', 'd1', 'd2', 'd3')


def _device_maps(x, dev):
    """numpy array, torch tensor or a list of [H, W] maps of either kind -> one contiguous float32 tensor on dev (device tensors that
    already are float32 and contiguous are used in place)."""
    import torch
    if isinstance(x, (list, tuple)):
        if len(x) and all(isinstance(m, torch.Tensor) for m in x):
            x = torch.stack([m.detach().to(dev, torch.float32) for m in x])
        else:
            x = np.stack([m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in x])
    if not isinstance(x, torch.Tensor):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())
    return x.detach().to(dev, torch.float32).contiguous()


def _evaluate_depth_device(depth_pred, depth_gt, depth_max, mode, device, scale_shift):
    import torch
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError(f"evaluate_depth(device={device!r}) runs HIP kernels on a gfx950 device; there is no CPU fallback "
                           "(leave device=None for the host path)")
    from .. import ops
    pred, gt = _device_maps(depth_pred, dev), _device_maps(depth_gt, dev)
    if pred.shape != gt.shape:
        raise ValueError(f"evaluate_depth: depth_pred {tuple(pred.shape)} and depth_gt {tuple(gt.shape)} differ in shape")
    if pred.numel() == 0:
        raise ValueError("no valid pixel: the maps are empty")
    if scale_shift is None:
        st, info = ops.depth_align(pred, gt, depth_max, mode)
    else:
        st = torch.tensor([float(scale_shift[0]), float(scale_shift[1])], dtype=torch.float64).to(dev)
    out = ops.depth_metrics(pred, gt, depth_max, st)
    vals = torch.cat([out, st]).cpu().numpy()          # the one read-back
    n_valid = int(vals[7])
    if n_valid < (2 if scale_shift is None else 1):
        raise ValueError(f"no valid pixel to evaluate on: {n_valid} of {pred.numel()} have 1e-3 < gt < {depth_max}")
    res = {k: float(v) for k, v in zip(METRIC_KEYS, vals[:7])}
    res.update(n_valid=n_valid, scale=float(vals[8]), shift=float(vals[9]))
    return res


def average_depth_metrics(results):
    """The n_valid-weighted average of per-sequence results (dicts of evaluate_depth): every metric key -> sum_k n_k m_k / sum_k n_k,
    n_valid -> the total (tool/depth_test.py:827-834)."""
    results = list(results)
    total = sum(int(r['n_valid']) for r in results)
    if not results or total <= 0:
        raise ValueError("average_depth_metrics: no valid pixel in any sequence")
    out = {k: float(sum(float(r[k]) * int(r['n_valid']) for r in results) / total) for k in METRIC_KEYS}
    out['n_valid'] = total
    return out


def evaluate_depth(depth_pred, depth_gt, depth_max=70.0, mode='lad', device=None, scale_shift=None):
    """depth_pred, depth_gt [T, H, W] (same size) -> dict(abs_rel, sq_rel, rmse, log_rmse, d1, d2, d3, n_valid).
    device='cuda' / 'cuda:k': the HIP path (csrc/metrics.hip).  The maps may be numpy arrays, torch tensors (device float32 tensors are
    used in place) or lists of [H, W] maps; they become float32, and validity is decided on those float32 values.  The dict then also
    holds `scale` and `shift`.  scale_shift=(s, t) skips the alignment rule and evaluates with the given pair (device path only)."""
    if device is not None:
        return _evaluate_depth_device(depth_pred, depth_gt, depth_max, mode, device, scale_shift)
    if scale_shift is not None:
        raise ValueError("evaluate_depth: scale_shift belongs to the device path (device='cuda')")
    depth_pred, depth_gt = np.asarray(depth_pred), np.asarray(depth_gt)
    valid = np.logical_and(depth_gt > 1e-3, depth_gt < depth_max)
    pred, gt = depth_pred[valid].astype(np.float64), depth_gt[valid].astype(np.float64)
    aligned = np.clip(align_depth(pred, gt, mode), 1e-5, depth_max)
    ratio = np.maximum(aligned / gt, gt / aligned)
    return dict(abs_rel=float(np.mean(np.abs(aligned - gt) / gt)), sq_rel=float(np.mean((aligned - gt) ** 2 / gt)),
                rmse=float(np.sqrt(np.mean((aligned - gt) ** 2))),
                log_rmse=float(np.sqrt(np.mean((np.log(aligned) - np.log(gt)) ** 2))),
                d1=float(np.mean(ratio < 1.25)), d2=float(np.mean(ratio < 1.25 ** 2)), d3=float(np.mean(ratio < 1.25 ** 3)),
                n_valid=int(valid.sum()))
