"""CPU (no GPU): the PLY writer / reader of align3r_amd/tool/pointcloud.py and the ctypes declarations of the scene-out entry
points (tests/test_lib_cpu.py compares the table with the header and the library's exports)."""
import ctypes as C
import os

import numpy as np
import pytest


def _cloud(M, seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((M, 3)).astype(np.float32)
    if M:
        xyz[0] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]      # signed zero, a denormal, near the largest float
    return xyz, rng.integers(0, 256, (M, 3), dtype=np.uint8)


HEAD_XYZ = "ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
HEAD_RGB = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


@pytest.mark.parametrize("with_rgb", [False, True], ids=["xyz", "xyz_rgb"])
@pytest.mark.parametrize("M", [0, 1, 1000])
def test_ply_header_length_and_bitwise_round_trip(M, with_rgb, tmp_path):
    from align3r_amd.tool.pointcloud import read_ply, write_ply
    xyz, rgb = _cloud(M)
    path = tmp_path / "c.ply"
    assert write_ply(path, xyz, rgb if with_rgb else None) == M
    data = path.read_bytes()
    head = (HEAD_XYZ.format(M) + (HEAD_RGB if with_rgb else "") + "end_header\n").encode("ascii")
    assert data[:len(head)] == head
    assert len(data) == len(head) + M * (15 if with_rgb else 12)
    if M:       # the first vertex, byte for byte: three little-endian floats, then three bytes
        assert data[len(head):len(head) + 12] == xyz[0].astype("<f4").tobytes()
        if with_rgb:
            assert data[len(head) + 12:len(head) + 15] == rgb[0].tobytes()
    x2, c2 = read_ply(path)
    assert x2.dtype == np.float32 and x2.shape == (M, 3)
    assert x2.tobytes() == xyz.tobytes()                        # bitwise (signed zero and the denormal included)
    if with_rgb:
        assert c2.dtype == np.uint8 and c2.shape == (M, 3) and np.array_equal(c2, rgb)
    else:
        assert c2 is None


def test_ply_parts_are_appended_in_order(tmp_path):
    from align3r_amd.tool.pointcloud import read_ply, write_ply_parts
    (a, ca), (b, cb), (e, ce) = _cloud(5, 1), _cloud(7, 2), _cloud(0, 3)
    assert write_ply_parts(tmp_path / "p.ply", [(a, ca), (e, ce), (b, cb)]) == 12
    xyz, rgb = read_ply(tmp_path / "p.ply")
    assert xyz.tobytes() == np.concatenate([a, b]).tobytes() and np.array_equal(rgb, np.concatenate([ca, cb]))
    assert write_ply_parts(tmp_path / "none.ply", []) == 0
    assert read_ply(tmp_path / "none.ply")[0].shape == (0, 3)
    with pytest.raises(ValueError, match="colours"):
        write_ply_parts(tmp_path / "bad.ply", [(a, ca), (b, None)])


def test_ply_refuses_wrong_shapes_and_dtypes(tmp_path):
    from align3r_amd.tool.pointcloud import read_ply, write_ply
    xyz, rgb = _cloud(4)
    for bad in (xyz.astype(np.float64), xyz[:, :2], xyz.reshape(-1), xyz.reshape(2, 2, 3)):
        with pytest.raises(ValueError, match="xyz"):
            write_ply(tmp_path / "x.ply", bad)
    for bad in (rgb.astype(np.int32), rgb[:3], rgb.astype(np.float32) / 255, rgb[:, :2]):
        with pytest.raises(ValueError, match="rgb"):
            write_ply(tmp_path / "x.ply", xyz, bad)
    (tmp_path / "junk.ply").write_bytes(b"not a ply file")
    with pytest.raises(ValueError):
        read_ply(tmp_path / "junk.ply")
    write_ply(tmp_path / "t.ply", xyz, rgb)
    (tmp_path / "trunc.ply").write_bytes((tmp_path / "t.ply").read_bytes()[:-1])
    with pytest.raises(ValueError):
        read_ply(tmp_path / "trunc.ply")


def test_scene_entry_points_are_declared():
    from align3r_amd import _lib
    names = ("a3r_align_scene_workspace_bytes", "a3r_align_scene_points", "a3r_align_scene_count", "a3r_align_scene_export")
    for name in names:
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["a3r_align_scene_workspace_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["a3r_align_scene_count"][1]) == 9 and len(_lib.SIGNATURES["a3r_align_scene_export"][1]) == 13
    lib = _lib.load()
    # host-side sizing and argument checks need no device: one int per 1024-pixel chunk of every image, plus the total
    assert lib.a3r_align_scene_workspace_bytes(16, 196608) >= (16 * 192 + 1) * 4
    assert lib.a3r_align_scene_workspace_bytes(3, 6) >= 16
    assert lib.a3r_align_scene_workspace_bytes(0, 6) == 0
    assert lib.a3r_align_scene_points(None, None, None) != 0
    total = C.c_longlong(-1)
    assert lib.a3r_align_scene_count(None, None, 0.0, None, None, 0, None, C.byref(total), None) != 0
    assert b"a3r_align_scene_count" in lib.a3r_last_error()
