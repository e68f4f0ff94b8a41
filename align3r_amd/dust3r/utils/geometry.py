"""Mirror of the two correspondence helpers of the reference's dust3r/utils/geometry.py: xy_grid and find_reciprocal_matches.

find_reciprocal_matches has two routes, split like tool/depth_metrics.evaluate_depth(device=):
  * host (numpy inputs, device=None; the default and the checker): two SciPy KD-trees, one nearest-neighbour query in each direction
    (workers=8) and the reciprocity test -- the reference's own route;
  * device (device='cuda', or CUDA tensors in): the exact brute-force search of csrc/match.hip through ops.reciprocal_matches.
    float64 distances from direct differences, the lowest index of a tie (include/a3r.h).  Where no two data points are at the
    same distance from a query the two routes return the same indices; at exact ties the KD-tree's choice depends on its
    traversal order, the device's is the lowest index.
"""
from __future__ import annotations

import numpy as np
import torch


def xy_grid(W, H, device=None, origin=(0, 0), unsqueeze=None, cat_dim=-1, homogeneous=False, **arange_kw):
    """Pixel coordinates of a W x H image: out[j, i] = (i + origin[0], j + origin[1]), x first.  numpy when device is None, torch on
    `device` otherwise.  homogeneous adds a plane of ones; unsqueeze inserts an axis into the x and y planes (torch only); cat_dim
    None returns the planes as a tuple instead of stacking them."""
    x0, y0 = origin
    if device is None:
        xs, ys = np.arange(x0, x0 + W, **arange_kw), np.arange(y0, y0 + H, **arange_kw)
        planes = tuple(np.meshgrid(xs, ys, indexing='xy'))
        if homogeneous:
            planes += (np.ones((H, W)),)
        stack = np.stack
    else:
        xs = torch.arange(x0, x0 + W, device=device, **arange_kw)
        ys = torch.arange(y0, y0 + H, device=device, **arange_kw)
        planes = tuple(torch.meshgrid(xs, ys, indexing='xy'))
        if homogeneous:
            planes += (torch.ones((H, W), device=device),)
        stack = torch.stack
    if unsqueeze is not None:
        planes = (planes[0].unsqueeze(unsqueeze), planes[1].unsqueeze(unsqueeze))
    return planes if cat_dim is None else stack(planes, cat_dim)


def _host_route(P1, P2):
    from scipy.spatial import cKDTree
    _, nn1_in_P2 = cKDTree(P2).query(P1, workers=8)
    _, nn2_in_P1 = cKDTree(P1).query(P2, workers=8)
    reciprocal_in_P2 = nn1_in_P2[nn2_in_P1] == np.arange(len(P2))
    return reciprocal_in_P2, nn2_in_P1, reciprocal_in_P2.sum()


def find_reciprocal_matches(P1, P2, device=None):
    """(reciprocal_in_P2 [n2] bool: P2[k2] and its nearest neighbour in P1 choose each other; nn2_in_P1 [n2]: the index of that
    neighbour; the number of matches).  P1 [n1,3], P2 [n2,3].  numpy arrays with device=None take the host route and return numpy
    values; device='cuda' (or a torch device), or CUDA tensors in, take the HIP kernels and return (bool tensor, int32 tensor, int)
    on that device."""
    on_device = lambda p: isinstance(p, torch.Tensor) and p.is_cuda
    if device is None and not (on_device(P1) or on_device(P2)):
        host = lambda p: p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        return _host_route(host(P1), host(P2))
    from ... import ops
    if device is None:
        device = P1.device if on_device(P1) else P2.device
    dev = lambda p: torch.as_tensor(p).to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    out = ops.reciprocal_matches(dev(P1), dev(P2))
    return out['reciprocal_in_P2'], out['nn2_in_P1'], out['count']
