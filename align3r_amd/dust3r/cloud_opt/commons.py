"""Small helpers of the global aligner (dust3r/cloud_opt/commons.py semantics)."""
import numpy as np
import torch

from ...aligner import cosine_schedule, linear_schedule  # noqa: F401  (commons.py:123-130)


def edge_str(i, j):
    return f'{i}_{j}'


def get_conf_trf(mode):          # commons.py:42-55
    if mode == 'log':
        return lambda x: x.log()
    if mode == 'sqrt':
        return lambda x: x.sqrt()
    if mode == 'm1':
        return lambda x: x - 1
    if mode in ('id', 'none'):
        return lambda x: x
    raise ValueError(f'bad mode for {mode=}')


def signed_log1p(x):             # commons.py:113-115
    return torch.sign(x) * torch.log1p(torch.abs(x))


def signed_expm1(x):             # commons.py:118-120
    return torch.sign(x) * torch.expm1(torch.abs(x))


def get_imshapes(edges, pred_i, pred_j):     # commons.py:27-39
    n_imgs = max(max(e) for e in edges) + 1
    imshapes = [None] * n_imgs
    for e, (i, j) in enumerate(edges):
        shape_i, shape_j = tuple(pred_i[e].shape[0:2]), tuple(pred_j[e].shape[0:2])
        if imshapes[i]:
            assert imshapes[i] == shape_i, f'incorrect shape for image {i}'
        if imshapes[j]:
            assert imshapes[j] == shape_j, f'incorrect shape for image {j}'
        imshapes[i], imshapes[j] = shape_i, shape_j
    return imshapes


def unitquat_to_rotmat(q):
    """XYZW unit quaternion -> rotation matrix (closed form used where the reference calls roma, base_opt.py:188)."""
    x, y, z, w = q.unbind(-1)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    rows = [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def rotmats_to_unitquats(R):
    """[B,3,3] rotation matrices (numpy) -> [B,4] XYZW unit quaternions, float32 (stands in for roma.rotmat_to_unitquat,
    base_opt.py:203): the numerically stable largest-component branch selection, in float64, every branch evaluated and one
    selected per matrix.  The package's one implementation of the formula."""
    R = np.asarray(R, dtype=np.float64)
    m = lambda i, j: R[:, i, j]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        s0 = np.sqrt(np.maximum(tr + 1.0, 1e-300)) * 2
        b0 = np.stack([(m(2, 1) - m(1, 2)) / s0, (m(0, 2) - m(2, 0)) / s0, (m(1, 0) - m(0, 1)) / s0, 0.25 * s0], -1)
        s1 = np.sqrt(np.maximum(1.0 + m(0, 0) - m(1, 1) - m(2, 2), 1e-300)) * 2
        b1 = np.stack([0.25 * s1, (m(0, 1) + m(1, 0)) / s1, (m(0, 2) + m(2, 0)) / s1, (m(2, 1) - m(1, 2)) / s1], -1)
        s2 = np.sqrt(np.maximum(1.0 + m(1, 1) - m(0, 0) - m(2, 2), 1e-300)) * 2
        b2 = np.stack([(m(0, 1) + m(1, 0)) / s2, 0.25 * s2, (m(1, 2) + m(2, 1)) / s2, (m(0, 2) - m(2, 0)) / s2], -1)
        s3 = np.sqrt(np.maximum(1.0 + m(2, 2) - m(0, 0) - m(1, 1), 1e-300)) * 2
        b3 = np.stack([(m(0, 2) + m(2, 0)) / s3, (m(1, 2) + m(2, 1)) / s3, 0.25 * s3, (m(1, 0) - m(0, 1)) / s3], -1)
    c0 = (tr > 0)[:, None]
    c1 = ((m(0, 0) > m(1, 1)) & (m(0, 0) > m(2, 2)))[:, None]
    c2 = (m(1, 1) > m(2, 2))[:, None]
    return np.where(c0, b0, np.where(c1, b1, np.where(c2, b2, b3))).astype(np.float32)


def rotmat_to_unitquat(R):
    """One rotation matrix (tensor, array or nested list) -> XYZW unit quaternion, a float32 CPU tensor."""
    return torch.from_numpy(rotmats_to_unitquats(torch.as_tensor(R, dtype=torch.float64).reshape(1, 3, 3).cpu().numpy())[0])
