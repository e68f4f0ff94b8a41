"""CPU (no GPU): the host side of the scene mesh -- mesh_faces_host (the plain-numpy statement of the definition in include/a3r.h)
against the reference's own pts3d_to_trimesh / cat_meshes (tests/golden/mesh.npz, written by tests/golden/make_goldens_mesh.py), and
the PLY mesh files of align3r_amd/tool/pointcloud.py.  Everything here is integer-valued: every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

META = json.load(open(os.path.join(GOLDEN, "mesh.json")))["cases"]


def load_case(name):
    """(valid maps, uint8 images, the reference's faces over the dense grids, the reference's face colours)"""
    g = np.load(os.path.join(GOLDEN, "mesh.npz"))
    c, n_img = META[name]["case"], len(META[name]["shapes"])
    return ([g[f"valid_{c}_{n}"] for n in range(n_img)], [g[f"img_{c}_{n}"] for n in range(n_img)], g[f"faces_{c}"], g[f"colors_{c}"])


def test_the_fixture_holds_the_cases_it_should():
    assert {"three_6x7", "mixed_6x8_8x6", "full_and_empty", "full_5x7"} <= set(META)
    assert META["three_6x7"]["shapes"] == [[6, 7]] * 3 and META["mixed_6x8_8x6"]["shapes"] == [[6, 8], [8, 6]]
    kept = META["full_and_empty"]["kept"]
    assert 42 in kept and 0 in kept
    assert META["full_5x7"]["faces"] == 4 * 4 * 6
    for name in ("three_6x7", "mixed_6x8_8x6"):                 # about 70 % kept, and faces of every kind to compare
        total = sum(h * w for h, w in META[name]["shapes"])
        assert 0.55 * total < sum(META[name]["kept"]) < 0.85 * total and META[name]["faces"] > 40


@pytest.mark.parametrize("name", list(META))
def test_host_faces_equal_the_reference(name):
    from align3r_amd.tool.pointcloud import mesh_faces_host
    valid, imgs, ref_faces, ref_colors = load_case(name)
    faces, colour = mesh_faces_host(valid, double_sided=True, index="dense")         # cumulative h * w offsets: the reference's
    assert faces.dtype == np.int32 and colour.dtype == np.int32
    assert np.array_equal(faces, ref_faces)
    flat = np.concatenate([im.reshape(-1, 3) for im in imgs])
    assert np.array_equal(flat[colour], ref_colors)
    # the rank form: every index replaced by the pixel's rank among the kept pixels
    keep = np.concatenate([v.ravel() for v in valid])
    rank = np.where(keep, np.cumsum(keep) - 1, -1)
    r_faces, r_colour = mesh_faces_host(valid, double_sided=True)
    assert np.array_equal(r_faces, rank[ref_faces]) and np.array_equal(r_colour, rank[colour])
    assert r_faces.size == 0 or (r_faces.min() >= 0 and r_faces.max() < keep.sum())
    assert np.array_equal(flat[keep][r_colour], ref_colors)
    # a dense numbering with a row stride (n * P + p)
    P = max(v.size for v in valid)
    s_faces, _ = mesh_faces_host(valid, double_sided=True, index="dense", stride=P)
    first = np.cumsum([0] + [v.size for v in valid])
    img_of = np.searchsorted(first, ref_faces, side="right") - 1
    assert np.array_equal(s_faces, ref_faces - first[img_of] + img_of * P)


@pytest.mark.parametrize("name", list(META))
def test_single_sided_is_the_a_b_subsequence(name):
    from align3r_amd.tool.pointcloud import mesh_faces_host
    valid, _, _, _ = load_case(name)
    two, two_c = mesh_faces_host(valid, double_sided=True)
    one, one_c = mesh_faces_host(valid, double_sided=False)
    assert len(two) == 2 * len(one)
    # per image [A, A', B, B'] against [A, B]: walk the images by their face counts
    at1 = at2 = 0
    for v in valid:
        (fa, _), (fb, _) = _blocks(v)
        for k in (fa, fb):
            assert np.array_equal(two[at2:at2 + k], one[at1:at1 + k]) and np.array_equal(two_c[at2:at2 + k], one_c[at1:at1 + k])
            assert np.array_equal(two[at2 + k:at2 + 2 * k], one[at1:at1 + k][:, ::-1])
            assert np.array_equal(two_c[at2 + k:at2 + 2 * k], one_c[at1:at1 + k])
            at1, at2 = at1 + k, at2 + 2 * k
    assert at1 == len(one) and at2 == len(two)


def _blocks(v):
    """((number of A triangles, their quads), (number of B triangles, their quads)) of one mask, by loops"""
    h, w = v.shape
    a = [(y, x) for y in range(h - 1) for x in range(w - 1) if v[y, x] and v[y, x + 1] and v[y + 1, x]]
    b = [(y, x) for y in range(h - 1) for x in range(w - 1) if v[y, x + 1] and v[y + 1, x] and v[y + 1, x + 1]]
    return (len(a), a), (len(b), b)


def test_host_faces_by_loops_on_an_odd_mask():
    """The definition spelled out with loops (no slicing), on a mask with a kept pixel in no triangle and a row end that must not
    wrap to the next row."""
    from align3r_amd.tool.pointcloud import mesh_faces_host
    v = np.array([[1, 1, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1], [0, 1, 1, 1]], bool)
    rank = (np.cumsum(v.ravel()) - 1).reshape(v.shape)
    (na, qa), (nb, qb) = _blocks(v)
    want = [(rank[y, x], rank[y, x + 1], rank[y + 1, x]) for y, x in qa] + [(rank[y, x + 1], rank[y + 1, x], rank[y + 1, x + 1]) for y, x in qb]
    col = [rank[y, x] for y, x in qa] + [rank[y + 1, x + 1] for y, x in qb]
    faces, colour = mesh_faces_host([v])
    assert np.array_equal(faces, np.asarray(want)) and np.array_equal(colour, col) and (na, nb) == (3, 3)
    assert rank[0, 3] not in faces                                   # kept, in no triangle: it stays a vertex all the same
    empty, ec = mesh_faces_host([np.zeros((3, 3), bool), np.eye(3, dtype=bool)])
    assert empty.shape == (0, 3) and ec.shape == (0,) and empty.dtype == np.int32
    assert mesh_faces_host([])[0].shape == (0, 3)
    assert len(mesh_faces_host([np.ones((1, 9), bool), np.ones((9, 1), bool)])[0]) == 0       # a single row / column has no quad
    with pytest.raises(ValueError):
        mesh_faces_host([v.astype(np.uint8)])
    with pytest.raises(ValueError):
        mesh_faces_host([v], index="pixel")


def _mesh(rng, V, F, colours):
    xyz = rng.standard_normal((V, 3)).astype(np.float32)
    if V > 3:
        xyz[1, 0], xyz[2, 1], xyz[3, 2] = np.nan, np.inf, -0.0                   # bits must survive
    faces = rng.integers(0, max(V, 1), (F, 3)).astype(np.int32)
    rgb = rng.integers(0, 256, (V, 3), dtype=np.uint8) if colours else None
    face_rgb = rng.integers(0, 256, (F, 3), dtype=np.uint8) if colours else None
    return xyz, faces, rgb, face_rgb


@pytest.mark.parametrize("V,F", [(50, 77), (9, 0), (0, 0)])
@pytest.mark.parametrize("colours", [False, True])
def test_ply_mesh_round_trip_is_bitwise(tmp_path, V, F, colours):
    from align3r_amd.tool.pointcloud import read_ply, read_ply_mesh, write_ply_mesh
    xyz, faces, rgb, face_rgb = _mesh(np.random.default_rng(V + F), V, F, colours)
    path = tmp_path / "m.ply"
    assert write_ply_mesh(path, xyz, faces, rgb, face_rgb) == (V, F)
    got = read_ply_mesh(path)
    assert got[0].tobytes() == xyz.tobytes() and got[0].shape == (V, 3) and got[0].dtype == np.float32
    assert np.array_equal(got[1], faces) and got[1].dtype == np.int32 and got[1].shape == (F, 3)
    if colours:
        assert np.array_equal(got[2], rgb) and np.array_equal(got[3], face_rgb) and got[2].dtype == got[3].dtype == np.uint8
    else:
        assert got[2] is None and got[3] is None
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert head[2] == f"element vertex {V}" and f"element face {F}" in head and "property list uchar int vertex_indices" in head
    size = V * (15 if colours else 12) + F * (16 if colours else 13)
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + size
    with pytest.raises(ValueError):                                  # the point-cloud reader keeps to its own layout
        read_ply(path)


def test_ply_mesh_mixed_colours(tmp_path):
    """Vertex colours without face colours and the other way round."""
    from align3r_amd.tool.pointcloud import read_ply_mesh, write_ply_mesh
    xyz, faces, rgb, face_rgb = _mesh(np.random.default_rng(1), 20, 11, True)
    write_ply_mesh(tmp_path / "v.ply", xyz, faces, rgb, None)
    got = read_ply_mesh(tmp_path / "v.ply")
    assert np.array_equal(got[2], rgb) and got[3] is None and np.array_equal(got[1], faces)
    write_ply_mesh(tmp_path / "f.ply", xyz, faces, None, face_rgb)
    got = read_ply_mesh(tmp_path / "f.ply")
    assert got[2] is None and np.array_equal(got[3], face_rgb) and got[0].tobytes() == xyz.tobytes()


def test_ply_mesh_parts_offset_the_indices(tmp_path):
    from align3r_amd.tool.pointcloud import read_ply_mesh, write_ply_mesh_parts
    rng = np.random.default_rng(3)
    a, e, b = _mesh(rng, 7, 5, True), _mesh(rng, 0, 0, True), _mesh(rng, 4, 6, True)
    assert write_ply_mesh_parts(tmp_path / "p.ply", [a, e, b]) == (11, 11)
    xyz, faces, rgb, face_rgb = read_ply_mesh(tmp_path / "p.ply")
    assert xyz.tobytes() == np.concatenate([a[0], b[0]]).tobytes() and np.array_equal(rgb, np.concatenate([a[2], b[2]]))
    assert np.array_equal(faces, np.concatenate([a[1], b[1] + 7])) and np.array_equal(face_rgb, np.concatenate([a[3], b[3]]))
    assert np.array_equal(a[1], _mesh(np.random.default_rng(3), 7, 5, True)[1])          # the inputs are left as they were
    assert write_ply_mesh_parts(tmp_path / "none.ply", []) == (0, 0)
    assert read_ply_mesh(tmp_path / "none.ply")[1].shape == (0, 3)
    with pytest.raises(ValueError, match="colours"):
        write_ply_mesh_parts(tmp_path / "bad.ply", [a, b[:2] + (None, None)])
    with pytest.raises(ValueError, match="colours"):
        write_ply_mesh_parts(tmp_path / "bad.ply", [a, b[:3] + (None,)])


def test_ply_mesh_refuses_bad_input(tmp_path):
    from align3r_amd.tool.pointcloud import read_ply_mesh, write_ply, write_ply_mesh
    xyz, faces, rgb, face_rgb = _mesh(np.random.default_rng(5), 10, 8, True)
    path = tmp_path / "x.ply"
    for bad in (faces.astype(np.int64), faces.astype(np.uint32), faces[:, :2], faces.reshape(-1)):
        with pytest.raises(ValueError, match="faces"):
            write_ply_mesh(path, xyz, bad)
    for bad in (face_rgb.astype(np.float32), face_rgb[:-1], face_rgb[:, :2]):
        with pytest.raises(ValueError, match="face_rgb"):
            write_ply_mesh(path, xyz, faces, rgb, bad)
    with pytest.raises(ValueError, match="xyz"):
        write_ply_mesh(path, xyz.astype(np.float64), faces)
    with pytest.raises(ValueError, match="rgb"):
        write_ply_mesh(path, xyz, faces, rgb[:-1])
    for v in (10, -1):
        bad = faces.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="index"):
            write_ply_mesh(path, xyz, bad)
    with pytest.raises(ValueError, match="index"):
        write_ply_mesh(path, xyz[:0], faces)
    # the mesh reader refuses a point-cloud file and a truncated mesh
    write_ply(path, xyz, rgb)
    with pytest.raises(ValueError):
        read_ply_mesh(path)
    write_ply_mesh(path, xyz, faces, rgb, face_rgb)
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-1])
    with pytest.raises(ValueError, match="bytes"):
        read_ply_mesh(path)


def test_the_c_table_names_the_mesh_entry_points():
    from align3r_amd import _lib
    sig = _lib.SIGNATURES
    assert len(sig["a3r_align_scene_mesh_workspace_bytes"][1]) == 2
    assert len(sig["a3r_align_scene_mesh_count"][1]) == 10 and len(sig["a3r_align_scene_mesh_export"][1]) == 17
    lib = _lib.load()
    rank_map = 3 * 1517 * 4
    assert lib.a3r_align_scene_mesh_workspace_bytes(3, 1517) >= rank_map + (1 + 4) * 3 * 2 * 4
    assert lib.a3r_align_scene_mesh_workspace_bytes(3, 1517) % 256 == 0
    assert lib.a3r_align_scene_mesh_workspace_bytes(0, 10) == 0 and lib.a3r_align_scene_mesh_workspace_bytes(2, 0) == 0
    # no handle: refused with the argument named, nothing touched
    nv, nf = C.c_longlong(-1), C.c_longlong(-1)
    buf = (C.c_float * 4)()
    assert lib.a3r_align_scene_mesh_count(None, buf, 1.0, None, buf, 16, 0, C.byref(nv), C.byref(nf), None) != 0
    assert lib.a3r_align_scene_mesh_export(None, buf, 1.0, None, None, buf, 16, 0, 0, 0, None, None, None, buf, C.byref(nv), C.byref(nf),
                                           None) != 0
    assert b"out_face_rgb needs the rgb" in lib.a3r_last_error()
