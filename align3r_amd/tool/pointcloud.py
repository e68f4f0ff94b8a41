"""Point-cloud files: binary little-endian PLY with `float x y z` and, optionally, `uchar red green blue` per vertex.

What the reference's tool/demo.py (get_3D_model_from_scene) hands to trimesh for its point-cloud export; written here directly
so that the output of PointCloudOptimizer.get_pointcloud() (device compaction, csrc/scene.hip) reaches a file every viewer opens.
"""
from __future__ import annotations

import numpy as np

_XYZ = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
_RGB = [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]


def ply_header(n_points: int, with_rgb: bool) -> bytes:
    lines = ['ply', 'format binary_little_endian 1.0', f'element vertex {int(n_points)}',
             'property float x', 'property float y', 'property float z']
    if with_rgb:
        lines += ['property uchar red', 'property uchar green', 'property uchar blue']
    lines.append('end_header')
    return ('\n'.join(lines) + '\n').encode('ascii')


def _check(xyz, rgb):
    xyz = np.asarray(xyz)
    if xyz.dtype != np.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f'xyz must be float32 [M,3], got {xyz.dtype} {xyz.shape}')
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
            raise ValueError(f'rgb must be uint8 {xyz.shape}, got {rgb.dtype} {rgb.shape}')
    return xyz, rgb


def _records(xyz, rgb):
    rec = np.empty(len(xyz), dtype=_XYZ + (_RGB if rgb is not None else []))       # packed: 12 or 15 bytes per vertex
    rec['x'], rec['y'], rec['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rec['red'], rec['green'], rec['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return rec


def write_ply(path, xyz, rgb=None):
    """xyz float32 [M,3], rgb uint8 [M,3] or None.  M = 0 writes a valid, empty cloud.  Returns M."""
    return write_ply_parts(path, [(xyz, rgb)])


def write_ply_parts(path, parts):
    """One PLY from several (xyz, rgb) clouds appended in order (the clips of the hierarchical driver); either every part has
    colours or none.  Returns the number of points."""
    parts = [_check(xyz, rgb) for xyz, rgb in parts]
    with_rgb = bool(parts) and parts[0][1] is not None
    if any((rgb is not None) != with_rgb for _, rgb in parts):
        raise ValueError('either every part of a point cloud has colours or none')
    total = sum(len(xyz) for xyz, _ in parts)
    with open(path, 'wb') as f:
        f.write(ply_header(total, with_rgb))
        for xyz, rgb in parts:
            f.write(_records(xyz, rgb).tobytes())
    return total


def read_ply(path):
    """(xyz float32 [M,3], rgb uint8 [M,3] or None) of a file written by write_ply (this vertex layout only)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    head = data[:end].decode('ascii').split('\n')[:-1]
    body = data[end + len(b'end_header\n'):]
    if head[1] != 'format binary_little_endian 1.0' or not head[2].startswith('element vertex '):
        raise ValueError(f'{path}: unsupported PLY header {head[:3]}')
    n = int(head[2].split()[2])
    props = head[3:]
    xyz_props = ['property float x', 'property float y', 'property float z']
    rgb_props = ['property uchar red', 'property uchar green', 'property uchar blue']
    if props == xyz_props:
        dtype = _XYZ
    elif props == xyz_props + rgb_props:
        dtype = _XYZ + _RGB
    else:
        raise ValueError(f'{path}: unsupported vertex properties {props}')
    rec = np.frombuffer(body, dtype=np.dtype(dtype))
    if len(rec) != n or len(body) != n * np.dtype(dtype).itemsize:
        raise ValueError(f'{path}: {len(body)} bytes of vertex data for {n} vertices')
    xyz = np.stack([rec['x'], rec['y'], rec['z']], axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    rgb = None
    if dtype is not _XYZ:
        rgb = np.stack([rec['red'], rec['green'], rec['blue']], axis=1).astype(np.uint8) if n else np.zeros((0, 3), np.uint8)
    return xyz, rgb
