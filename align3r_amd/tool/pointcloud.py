"""Point-cloud files: binary little-endian PLY with `float x y z` and, optionally, `uchar red green blue` per vertex.

What the reference's tool/demo.py (get_3D_model_from_scene) hands to trimesh for its point-cloud export; written here directly
so that the output of PointCloudOptimizer.get_pointcloud() (device compaction, csrc/scene.hip) reaches a file every viewer opens.

Mesh files: the same vertex element followed by `element face F` (`property list uchar int vertex_indices`, optionally
`uchar red green blue` per face) -- the reference's default scene output (pts3d_to_trimesh / cat_meshes of dust3r/viz.py), here
the output of PointCloudOptimizer.get_mesh().  mesh_faces_host states the face rule in numpy: the checker of the device path.
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


_FACE = [('n', 'u1'), ('v', '<i4', (3,))]
_FACE_PROPS = ['property list uchar int vertex_indices']
_RGB_PROPS = ['property uchar red', 'property uchar green', 'property uchar blue']


def _check_mesh(xyz, faces, rgb, face_rgb):
    xyz, rgb = _check(xyz, rgb)
    faces = np.asarray(faces)
    if faces.dtype != np.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f'faces must be int32 [F,3], got {faces.dtype} {faces.shape}')
    if faces.size and (faces.min() < 0 or faces.max() >= len(xyz)):
        raise ValueError(f'faces index vertices {int(faces.min())} .. {int(faces.max())} of {len(xyz)}')
    if face_rgb is not None:
        face_rgb = np.asarray(face_rgb)
        if face_rgb.dtype != np.uint8 or face_rgb.shape != faces.shape:
            raise ValueError(f'face_rgb must be uint8 {faces.shape}, got {face_rgb.dtype} {face_rgb.shape}')
    return xyz, faces, rgb, face_rgb


def write_ply_mesh(path, xyz, faces, rgb=None, face_rgb=None):
    """A triangle mesh as a binary little-endian PLY: the vertex element of write_ply (xyz float32 [V,3], rgb uint8 [V,3] or None),
    then `element face F` with `property list uchar int vertex_indices` (faces int32 [F,3], every index below V) and, with
    face_rgb uint8 [F,3], `uchar red green blue` per face.  V = 0 and F = 0 write valid, empty elements.  Returns (V, F)."""
    return write_ply_mesh_parts(path, [(xyz, faces, rgb, face_rgb)])


def write_ply_mesh_parts(path, parts):
    """One PLY from several (xyz, faces, rgb, face_rgb) meshes appended in order (the clips of the hierarchical driver): every
    part's faces index its own vertices and are written with the part's vertex offset added.  Either every part has vertex (face)
    colours or none.  Returns (V, F)."""
    parts = [_check_mesh(*part) for part in parts]
    with_rgb = bool(parts) and parts[0][2] is not None
    with_face_rgb = bool(parts) and parts[0][3] is not None
    if any((p[2] is not None) != with_rgb or (p[3] is not None) != with_face_rgb for p in parts):
        raise ValueError('either every part of a mesh has vertex (face) colours or none')
    V, F = sum(len(p[0]) for p in parts), sum(len(p[1]) for p in parts)
    if V >= 2 ** 31:
        raise ValueError(f'{V} vertices do not fit the int32 indices of the face element')
    head = ply_header(V, with_rgb).decode('ascii').split('\n')[:-2]
    head += [f'element face {F}'] + _FACE_PROPS + (_RGB_PROPS if with_face_rgb else []) + ['end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(head) + '\n').encode('ascii'))
        for xyz, _, rgb, _ in parts:
            f.write(_records(xyz, rgb).tobytes())
        offset = 0
        for xyz, faces, _, face_rgb in parts:
            rec = np.empty(len(faces), dtype=_FACE + (_RGB if with_face_rgb else []))      # packed: 13 or 16 bytes per face
            rec['n'], rec['v'] = 3, faces + np.int32(offset)
            if with_face_rgb:
                rec['red'], rec['green'], rec['blue'] = face_rgb[:, 0], face_rgb[:, 1], face_rgb[:, 2]
            f.write(rec.tobytes())
            offset += len(xyz)
    return V, F


def read_ply_mesh(path):
    """(xyz float32 [V,3], faces int32 [F,3], rgb uint8 [V,3] or None, face_rgb uint8 [F,3] or None) of a file written by
    write_ply_mesh (this layout only: triangles, int32 indices)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    head = data[:end].decode('ascii').split('\n')[:-1]
    body = data[end + len(b'end_header\n'):]
    elems = [k for k, line in enumerate(head) if line.startswith('element ')]
    if (head[1] != 'format binary_little_endian 1.0' or len(elems) != 2 or elems[0] != 2 or not head[2].startswith('element vertex ')
            or not head[elems[1]].startswith('element face ')):
        raise ValueError(f'{path}: not a vertex + face PLY of this module')
    V, F = int(head[2].split()[2]), int(head[elems[1]].split()[2])
    vprops, fprops = head[3:elems[1]], head[elems[1] + 1:]
    xyz_props = ['property float x', 'property float y', 'property float z']
    if vprops not in (xyz_props, xyz_props + _RGB_PROPS) or fprops not in (_FACE_PROPS, _FACE_PROPS + _RGB_PROPS):
        raise ValueError(f'{path}: unsupported properties {vprops} / {fprops}')
    vtype = np.dtype(_XYZ + (_RGB if len(vprops) > 3 else []))
    ftype = np.dtype(_FACE + (_RGB if len(fprops) > 1 else []))
    if len(body) != V * vtype.itemsize + F * ftype.itemsize:
        raise ValueError(f'{path}: {len(body)} bytes of data for {V} vertices and {F} faces')
    vrec = np.frombuffer(body, dtype=vtype, count=V)
    frec = np.frombuffer(body, dtype=ftype, count=F, offset=V * vtype.itemsize)
    if F and (frec['n'] != 3).any():
        raise ValueError(f'{path}: a face that is no triangle')
    colours = lambda rec: np.stack([rec['red'], rec['green'], rec['blue']], axis=1).astype(np.uint8).reshape(-1, 3)
    xyz = np.stack([vrec['x'], vrec['y'], vrec['z']], axis=1).astype(np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(frec['v']).astype(np.int32).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f'{path}: faces index vertices {int(faces.min())} .. {int(faces.max())} of {V}')
    return xyz, faces, (colours(vrec) if len(vprops) > 3 else None), (colours(frec) if len(fprops) > 1 else None)


def mesh_faces_host(valid_list, double_sided=False, index='rank', stride=None):
    """The triangles of the scene mesh (include/a3r.h: a3r_align_scene_mesh_export) from the kept masks alone, in plain numpy: the
    checker of the device path.  valid_list: one bool [h,w] map per image.  Per image and per pixel quad with the corners
    tl = (y,x), tr = (y,x+1), bl = (y+1,x), br = (y+1,x+1): A = (tl,tr,bl) where those three are kept, B = (tr,bl,br) where those
    are; all A in row-major quad order, then all B; double_sided puts each block's triangles wound backwards right after it
    ([A, A', B, B']).  Returns (faces int32 [F,3], colour int32 [F]): the vertices of every face and the pixel that gives the face
    its colour (tl for A, br for B), both as
      index='rank'  : the pixel's rank among the kept pixels of the whole scene (image-major, row-major) -- the device's vertex ids;
      index='dense' : n * stride + y * w + x, or with stride=None the image's cumulative offset sum(h * w of the images before) +
                      y * w + x (the numbering of a concatenation of the full grids)."""
    if index not in ('rank', 'dense'):
        raise ValueError(f"index must be 'rank' or 'dense', got {index!r}")
    faces, colour, first = [], [], 0
    for n, valid in enumerate(valid_list):
        valid = np.asarray(valid)
        if valid.dtype != np.bool_ or valid.ndim != 2:
            raise ValueError(f'valid_list[{n}] must be bool [h,w], got {valid.dtype} {valid.shape}')
        h, w = valid.shape
        if index == 'rank':
            ids = np.full(h * w, -1, np.int64)
            kept = int(valid.sum())
            ids[valid.ravel()] = first + np.arange(kept)
            first += kept
        else:
            ids = (n * stride if stride is not None else first) + np.arange(h * w, dtype=np.int64)
            first += h * w
        ids = ids.reshape(h, w)
        tl, tr, bl, br = ids[:-1, :-1], ids[:-1, 1:], ids[1:, :-1], ids[1:, 1:]
        diag = valid[:-1, 1:] & valid[1:, :-1]
        has_a, has_b = diag & valid[:-1, :-1], diag & valid[1:, 1:]
        a = np.stack([tl[has_a], tr[has_a], bl[has_a]], axis=1)
        b = np.stack([tr[has_b], bl[has_b], br[has_b]], axis=1)
        for tri, col in ((a, tl[has_a]), (b, br[has_b])):
            faces.append(tri)
            colour.append(col)
            if double_sided:
                faces.append(tri[:, ::-1])
                colour.append(col)
    if first >= 2 ** 31:
        raise ValueError(f'{first} vertices do not fit int32')
    cat = lambda parts, shape: np.concatenate(parts).astype(np.int32) if parts else np.zeros(shape, np.int32)
    return cat(faces, (0, 3)), cat(colour, (0,))


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
