"""GPU: point correspondences (csrc/match.hip) -- exact 3-D nearest neighbours and reciprocal matches.

The kernels have no tolerance: every index, every flag, every pair and the bits of every squared distance are compared with
  * brute(), the float64 numpy restatement of the definition (tests/match_cases.py), on all kinds, and
  * the host route of find_reciprocal_matches (two KD-trees, the reference's own function) on the tie-free kinds, where
    tests/test_matches_cpu.py shows the two checkers to agree.
Sizes (1,1) .. (8193,8191): fewer points than a wave, ragged tiles, ragged query blocks, one more than 8 query blocks / 16 tiles.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import match_cases as mc

pytestmark = pytest.mark.gpu

SIZE_IDS = [f"{a}x{b}" for a, b in mc.SIZES]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_matches(got, ref):
    """every output of ops.reciprocal_matches against a restatement dict (match_cases.brute_case layout)"""
    assert got["nn2_in_P1"].dtype == torch.int32 and np.array_equal(host(got["nn2_in_P1"]), ref["nn2_in_P1"])
    assert got["nn1_in_P2"].dtype == torch.int32 and np.array_equal(host(got["nn1_in_P2"]), ref["nn1_in_P2"])
    assert got["reciprocal_in_P2"].dtype == torch.bool and np.array_equal(host(got["reciprocal_in_P2"]), ref["reciprocal_in_P2"])
    assert got["count"] == len(ref["pairs"])
    assert got["pairs"].dtype == torch.int32 and got["pairs"].shape == ref["pairs"].shape
    assert np.array_equal(host(got["pairs"]), ref["pairs"])


@pytest.mark.parametrize("sizes", mc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_nn_search_equals_brute(kind, sizes):
    from align3r_amd import ops
    ref = mc.brute_case(kind, *sizes)
    P1, P2 = dev(ref["P1"]), dev(ref["P2"])
    for q, d, idx, d2 in ((P2, P1, ref["nn2_in_P1"], ref["d2_2"]), (P1, P2, ref["nn1_in_P2"], ref["d2_1"])):
        got_i, got_d = ops.nn_search(q, d, return_dist=True)
        assert got_i.dtype == torch.int32 and got_d.dtype == torch.float64
        assert np.array_equal(host(got_i), idx)
        assert same_bits(host(got_d), d2)
        assert torch.equal(ops.nn_search(q, d), got_i)          # without the distances


@pytest.mark.parametrize("sizes", mc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", mc.TIE_FREE)
def test_reciprocal_matches_equal_the_host_route(kind, sizes):
    from align3r_amd import ops
    from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches
    P1, P2 = mc.pair(kind, *sizes)
    rec, nn2, count = find_reciprocal_matches(P1, P2)           # two KD-trees on the host
    got = ops.reciprocal_matches(dev(P1), dev(P2))
    assert np.array_equal(host(got["reciprocal_in_P2"]), rec)
    assert np.array_equal(host(got["nn2_in_P1"]), nn2)
    assert got["count"] == int(count)
    k2 = np.flatnonzero(rec)
    assert np.array_equal(host(got["pairs"]), np.stack([nn2[k2], k2], 1))
    check_matches(got, mc.brute_case(kind, *sizes))


@pytest.mark.parametrize("sizes", mc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", mc.TIE_RICH)
def test_reciprocal_matches_on_tie_rich_clouds_equal_brute(kind, sizes):
    from align3r_amd import ops
    ref = mc.brute_case(kind, *sizes)
    check_matches(ops.reciprocal_matches(dev(ref["P1"]), dev(ref["P2"])), ref)


@pytest.mark.parametrize("sizes", [(1000, 1337), (4099, 5)], ids=["1000x1337", "4099x5"])
@pytest.mark.parametrize("kind", mc.TIE_RICH)
def test_result_does_not_depend_on_chunks(kind, sizes):
    """Ties straddle every range boundary of these clouds; the lowest index must win whatever the cut.  64 ranges against 5 data
    points leaves most ranges empty."""
    from align3r_amd import ops
    ref = mc.brute_case(kind, *sizes)
    P1, P2 = dev(ref["P1"]), dev(ref["P2"])
    base = [ops.nn_search(P2, P1, return_dist=True), ops.nn_search(P1, P2, return_dist=True)]
    base_m = ops.reciprocal_matches(P1, P2)
    check_matches(base_m, ref)
    for chunks in (1, 2, 3, 7, 64):
        assert ops.nn_chunks(sizes[0], sizes[1], chunks) == chunks
        for (bi, bd), (q, d) in zip(base, ((P2, P1), (P1, P2))):
            gi, gd = ops.nn_search(q, d, chunks=chunks, return_dist=True)
            assert torch.equal(gi, bi), chunks
            assert same_bits(host(gd), host(bd)), chunks
        m = ops.reciprocal_matches(P1, P2, chunks=chunks)
        assert m["count"] == base_m["count"]
        for k in ("nn2_in_P1", "nn1_in_P2", "reciprocal_in_P2", "pairs"):
            assert torch.equal(m[k], base_m[k]), (chunks, k)


def test_non_finite_points_never_match():
    """NaN and +-inf coordinates in both sets: such a query gets (-1, +inf), such a data point is never returned and never reciprocal;
    everything else equals brute() on the clean subsets, mapped back."""
    from align3r_amd import ops
    P1, P2 = (p.copy() for p in mc.pair("uniform", 1000, 1337))
    g = np.random.default_rng(5)
    for P in (P1, P2):
        rows = g.choice(len(P), 90, replace=False)
        P[rows, g.integers(0, 3, 90)] = np.repeat(np.array([np.nan, np.inf, -np.inf], np.float32), 30)
    P1[7] = np.nan
    P2[0] = (np.inf, -np.inf, np.nan)
    ok1, ok2 = np.isfinite(P1).all(1), np.isfinite(P2).all(1)
    c1, c2 = np.flatnonzero(ok1), np.flatnonzero(ok2)
    assert 900 <= len(c1) < 1000 and 1200 <= len(c2) < 1337

    def expected(Q, okq, D, cd):
        idx, d2 = np.full(len(Q), -1, np.int32), np.full(len(Q), np.inf)
        i, d = mc.brute(Q[okq], D[cd])
        idx[okq], d2[okq] = cd[i], d
        return idx, d2

    nn2, d22 = expected(P2, ok2, P1, c1)
    nn1, d21 = expected(P1, ok1, P2, c2)
    rec, pairs = mc.reciprocal(nn2, nn1)
    D1, D2 = dev(P1), dev(P2)
    gi, gd = ops.nn_search(D2, D1, return_dist=True)
    assert np.array_equal(host(gi), nn2) and same_bits(host(gd), d22)
    assert (host(gi)[~ok2] == -1).all() and np.isposinf(host(gd)[~ok2]).all() and ok1[host(gi)[ok2]].all()
    gi, gd = ops.nn_search(D1, D2, return_dist=True)
    assert np.array_equal(host(gi), nn1) and same_bits(host(gd), d21)
    got = ops.reciprocal_matches(D1, D2)
    check_matches(got, dict(nn2_in_P1=nn2, nn1_in_P2=nn1, reciprocal_in_P2=rec, pairs=pairs))
    assert not host(got["reciprocal_in_P2"])[~ok2].any()
    assert ok1[host(got["pairs"])[:, 0]].all() and ok2[host(got["pairs"])[:, 1]].all()
    # a data set of non-finite points only is an empty one
    gi, gd = ops.nn_search(D2, dev(P1[~ok1]), return_dist=True)
    assert (host(gi) == -1).all() and np.isposinf(host(gd)).all()


@pytest.mark.parametrize("n1, n2", [(0, 37), (37, 0), (0, 0)])
def test_empty_sets(n1, n2):
    from align3r_amd import ops
    P1, P2 = (dev(p) for p in mc.pair("uniform", n1, n2))
    gi, gd = ops.nn_search(P2, P1, return_dist=True)
    assert gi.shape == (n2,) and (gi == -1).all() and torch.isposinf(gd).all()
    gi, gd = ops.nn_search(P1, P2, return_dist=True)
    assert gi.shape == (n1,) and (gi == -1).all() and torch.isposinf(gd).all()
    m = ops.reciprocal_matches(P1, P2)
    assert m["count"] == 0 and m["pairs"].shape == (0, 2)
    assert m["nn2_in_P1"].shape == (n2,) and (m["nn2_in_P1"] == -1).all()
    assert m["nn1_in_P2"].shape == (n1,) and (m["nn1_in_P2"] == -1).all()
    assert m["reciprocal_in_P2"].shape == (n2,) and not m["reciprocal_in_P2"].any()


def test_capacity_and_sentinels_through_the_c_entry():
    """capacity = M + 3: the tail keeps its sentinel.  capacity = M - 1: A3R_EINVAL with the needed count, and no pair was written."""
    from align3r_amd import _lib
    from align3r_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    ref = mc.brute_case("surface", 1000, 1337)
    P1, P2 = dev(ref["P1"]), dev(ref["P2"])
    n1, n2, M = 1000, 1337, len(ref["pairs"])
    assert M > 64
    ws_bytes = int(lib.a3r_match_workspace_bytes(n1, n2, 0))
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device="cuda")          # room for the misaligned call below
    nn2, nn1 = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (n2, n1))
    rec = torch.full((n2,), 0xAB, dtype=torch.uint8, device="cuda")

    def call(cap, pairs, nn1_out=nn1, wsb=ws_bytes, chunks=0):
        n = C.c_longlong(-1)
        rc = lib.a3r_reciprocal_matches(ptr(P1), n1, ptr(P2), n2, chunks, ptr(ws), wsb, ptr(nn2), ptr(nn1_out), ptr(rec), cap, ptr(pairs),
                                        C.byref(n), stream_ptr())
        torch.cuda.synchronize()
        return rc, n.value

    pairs = torch.full((M + 3, 2), -9, dtype=torch.int32, device="cuda")
    rc, n = call(M + 3, pairs)
    check(rc)
    assert n == M and np.array_equal(host(pairs[:M]), ref["pairs"]) and (pairs[M:] == -9).all()
    assert np.array_equal(host(nn2), ref["nn2_in_P1"]) and np.array_equal(host(nn1), ref["nn1_in_P2"])
    assert np.array_equal(host(rec), ref["reciprocal_in_P2"].astype(np.uint8))
    # one pair short
    pairs = torch.full((M - 1, 2), -9, dtype=torch.int32, device="cuda")
    rc, n = call(M - 1, pairs)
    assert rc == -1 and n == M                                  # A3R_EINVAL, the needed count
    msg = lib.a3r_last_error().decode()
    assert "capacity" in msg and str(M) in msg, msg
    assert (pairs == -9).all()
    # the count alone: no pair buffer, no nn1 output, the capacity is not looked at
    rc, n = call(0, None, nn1_out=None)
    check(rc)
    assert n == M
    # refusals before anything is launched
    rec.fill_(0xAB)
    for bad in (dict(wsb=ws_bytes - 1), dict(chunks=-1), dict(cap=-1)):
        kw = dict(cap=M, pairs=pairs)
        kw.update(bad)
        rc, n = call(**kw)
        assert rc == -1 and n == 0, bad
    assert lib.a3r_reciprocal_matches(ptr(P1), n1, ptr(P2), n2, 0, C.c_void_p(ws.data_ptr() + 4), ws_bytes, ptr(nn2), None, ptr(rec), 0, None,
                                      C.byref(C.c_longlong()), stream_ptr()) == -1
    assert "aligned" in lib.a3r_last_error().decode()
    assert lib.a3r_reciprocal_matches(None, n1, ptr(P2), n2, 0, ptr(ws), ws_bytes, ptr(nn2), None, ptr(rec), 0, None,
                                      C.byref(C.c_longlong()), stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (rec == 0xAB).all()


def test_same_call_twice_gives_the_same_bytes():
    from align3r_amd import ops
    ref = mc.brute_case("lattice", 8193, 8191)
    P1, P2 = dev(ref["P1"]), dev(ref["P2"])
    a, b = ops.reciprocal_matches(P1, P2), ops.reciprocal_matches(P1, P2)
    assert a["count"] == b["count"]
    for k in ("nn2_in_P1", "nn1_in_P2", "reciprocal_in_P2", "pairs"):
        assert same_bits(host(a[k]), host(b[k])), k
    (i1, d1), (i2, d2) = ops.nn_search(P2, P1, return_dist=True), ops.nn_search(P2, P1, return_dist=True)
    assert same_bits(host(i1), host(i2)) and same_bits(host(d1), host(d2))


def test_many_workgroups_on_both_grid_axes():
    """surface (36 864, 36 864): 36 query blocks, and the library cuts the data into several ranges; against the host route."""
    from align3r_amd import ops
    from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches
    n = 36864
    assert ops.nn_chunks(n, n) > 1
    P1, P2 = mc.pair("surface", n, n)
    rec, nn2, count = find_reciprocal_matches(P1, P2)
    _, nn1, _ = find_reciprocal_matches(P2, P1)
    got = ops.reciprocal_matches(dev(P1), dev(P2))
    assert np.array_equal(host(got["reciprocal_in_P2"]), rec)
    assert np.array_equal(host(got["nn2_in_P1"]), nn2) and np.array_equal(host(got["nn1_in_P2"]), nn1)
    assert got["count"] == int(count) > 1000
    k2 = np.flatnonzero(rec)
    assert np.array_equal(host(got["pairs"]), np.stack([nn2[k2], k2], 1))


def test_find_reciprocal_matches_on_the_device_equals_the_default_route():
    from align3r_amd.dust3r.utils.geometry import find_reciprocal_matches
    P1, P2 = mc.pair("surface", 1000, 1337)
    rec, nn2, count = find_reciprocal_matches(P1, P2)
    for a, b, kw in ((P1, P2, dict(device="cuda")), (dev(P1), dev(P2), {}), (dev(P1), P2, {})):
        r, n, c = find_reciprocal_matches(a, b, **kw)
        assert r.is_cuda and r.dtype == torch.bool and n.is_cuda
        assert np.array_equal(host(r), rec) and np.array_equal(host(n), nn2) and int(c) == int(count)


# ------------------------------------------------------------------------------------------------- scene.get_matches
def _scene(name):
    import test_gpu_scene as tgs                                # the scene builders of the scene-out tests, as they are
    if name == "mixed":
        return tgs.make_mixed_scene()[0]
    return tgs.make_scene(name, 4 if name == "flow" else 3, 36, 44)[0]


@pytest.mark.parametrize("name, pairs_ij, quantile, kw", [
    ("plain", [(0, 1), (2, 0)], 0.5, {}),
    ("plain", [(1, 2)], None, {}),                              # min_conf_thr=None: the scene's own threshold, the pixels of get_masks()
    ("flow", [(0, 1), (2, 1)], 0.25, dict(mask_dynamic=True)),
    ("mixed", [(0, 1), (1, 2), (3, 1)], 0.5, {}),               # 32x48 against 24x40: each image's own width
], ids=["plain", "plain_default_thr", "flow_masked", "mixed"])
def test_scene_get_matches_equals_brute_on_the_exported_cloud(name, pairs_ij, quantile, kw):
    """The threshold is a quantile of the scene's own confidences, so that every image keeps a known share of its pixels."""
    scene = _scene(name)
    if quantile is not None:
        kw = dict(kw, min_conf_thr=float(np.quantile(np.concatenate([host(c).ravel() for c in scene.im_conf]), quantile)))
    pc = scene.get_pointcloud(with_index=True, **kw)
    index, xyz, P = host(pc["index"]), host(pc["xyz"]), scene.max_area
    for i, j in pairs_ij:
        rows_i, rows_j = np.flatnonzero(index // P == i), np.flatnonzero(index // P == j)
        assert quantile is None or (len(rows_i) > 50 and len(rows_j) > 50)
        Pi, Pj = xyz[rows_i], xyz[rows_j]
        nn2, _ = mc.brute(Pj, Pi)
        nn1, _ = mc.brute(Pi, Pj)
        _, pairs = mc.reciprocal(nn2, nn1)
        got = scene.get_matches(i, j, **kw)
        assert got["count"] == len(pairs) and (quantile is None or len(pairs) > 0)
        want_i, want_j = index[rows_i][pairs[:, 0]] - i * P, index[rows_j][pairs[:, 1]] - j * P
        assert (np.diff(want_j) > 0).all()                      # ascending order of image j's kept pixels
        for key, want, n in (("i", want_i, i), ("j", want_j, j)):
            h, w = scene.imshapes[n]
            assert got["idx_" + key].dtype == torch.int32 and np.array_equal(host(got["idx_" + key]), want)
            assert (want < h * w).all()
            assert got["xy_" + key].dtype == torch.int32 and got["xy_" + key].shape == (len(pairs), 2)
            assert np.array_equal(host(got["xy_" + key]), np.stack([want % w, want // w], 1))
        assert same_bits(host(got["xyz_i"]), Pi[pairs[:, 0]]) and same_bits(host(got["xyz_j"]), Pj[pairs[:, 1]])


def test_scene_get_matches_refuses_bad_indices():
    scene = _scene("plain")
    with pytest.raises(ValueError):
        scene.get_matches(1, 1)
    for i, j in ((0, 3), (3, 0), (-1, 0), (0, 17)):
        with pytest.raises(IndexError):
            scene.get_matches(i, j)
    with pytest.raises(RuntimeError, match="dynamic masks"):
        scene.get_matches(0, 1, mask_dynamic=True)              # a plain scene has none


def test_run_clip_writes_one_file_per_consecutive_pair(tmp_path):
    from align3r_amd.tool.run_clip import write_matches
    scene = _scene("mixed")
    counts = write_matches(scene, str(tmp_path / "m"))
    assert len(counts) == scene.n_imgs - 1
    for i, c in enumerate(counts):
        f = np.load(tmp_path / "m" / f"matches_{i}_{i + 1}.npz")
        want = scene.get_matches(i, i + 1)
        assert sorted(f.files) == sorted(want) and int(f["count"]) == c == want["count"]
        for k in ("idx_i", "idx_j", "xy_i", "xy_j", "xyz_i", "xyz_j"):
            assert same_bits(f[k], host(want[k])), k
