"""CPU: the motion-mask oracle of tests/motion_cases.py against the reference's golden (tests/golden/motion.npz) and against the
package's torch checker (cloud_opt_flow.optimizer.motion_masks_torch) with injected geometry; the host-built entry table; the mask /
confidence writers, enlarge_seg_masks and the refusals of run_clip --flow.  Flagged and masked shares per scene are printed
(DESIGN 6.6)."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import motion_cases as mc
from conftest import GOLDEN, record_margin


def _entries(sc):
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_entries
    return motion_entries(sc["geom"], sc["edges"], len(sc["edges"]))


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, (N, graph, H, W, kw) in mc.SCENES.items():
        sc = mc.make_scene(N, graph, H, W, **kw)
        sc["entries"] = _entries(sc)
        sc["oracle"] = mc.oracle(sc["entries"], sc["pred_i"], sc["pred_j"], sc["flow_ij"], sc["flow_ji"], sc["lists"], H, W)
        out[name] = sc
    return out


def test_entry_layout_and_lists_agree_with_the_package():
    from align3r_amd import _lib, ops
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_vote_lists
    import ctypes as C
    assert ops.MOTION_ENTRY == mc.ENTRY and mc.ENTRY.itemsize == C.sizeof(_lib.MotionEntry) == 80
    edges = [(0, 1), (1, 2), (0, 2), (1, 0), (2, 1), (2, 0)]
    assert motion_vote_lists(edges, 3) == mc.vote_lists(edges, 3) == [[0, 2], [3, 1], [4, 5]]


def test_oracle_reproduces_the_reference_golden():
    """motion.npz: the reference's own get_motion_mask_from_pairs with a PairViewer stand-in that returned the stored geometry."""
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_entries, motion_masks_torch
    g = np.load(os.path.join(GOLDEN, "motion.npz"))
    edges = [tuple(int(v) for v in e) for e in g["edges"]]
    N, H, W = g["masks"].shape
    E = len(edges)
    geom = dict(K_i=g["K_i"], K_j=g["K_j"], pose_i=g["pose_i"], pose_j=g["pose_j"], depth_i=(g["depth_row_i"], g["depth_rt_i"]),
                depth_j=(g["depth_row_j"], g["depth_rt_j"]))
    # the stored depth descriptors are the stored depth maps
    pts = np.concatenate([g["pred_i"], g["pred_j"]])
    for (row, rt), D in ((geom["depth_i"], g["D_i"]), (geom["depth_j"], g["D_j"])):
        for r, t, d in zip(row, rt, D):
            assert np.allclose(pts[r] @ t[:3] + t[3], d, rtol=0, atol=1e-5)
    lists = mc.vote_lists(edges, N)
    mean, mask, flagged, info = mc.oracle(motion_entries(geom, edges, E), g["pred_i"], g["pred_j"], g["flow_ij"], g["flow_ji"], lists, H, W,
                                          float(g["thre"]))
    mc.assert_cap(info, mask)
    differ = mc.check_agreement(g["masks"], None, mean, mask, flagged, info)
    record_margin("motion_golden", flagged_share=info["flagged"], masked_share=info["masked"], flagged_differing=differ)
    # and the package's torch function on the stored geometry is the reference bit for bit
    t = torch.from_numpy
    masks, _ = motion_masks_torch(edges, N, t(g["K_i"]), t(g["K_j"]), t(g["pose_i"][:, :3, :3]), t(g["pose_j"][:, :3, :3]),
                                  t(g["pose_i"][:, :3, 3:]), t(g["pose_j"][:, :3, 3:]), t(g["D_i"]), t(g["D_j"]), t(g["flow_ij"]),
                                  t(g["flow_ji"]), float(g["thre"]))
    assert np.array_equal(torch.stack(masks).numpy(), g["masks"])


@pytest.mark.parametrize("name", list(mc.SCENES))
def test_oracle_keeps_every_scene_within_the_cap_and_torch_agrees(scenes, name):
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import motion_masks_torch
    sc = scenes[name]
    mean, mask, flagged, info = sc["oracle"]
    mc.assert_cap(info, mask)
    assert not info["nan_images"]
    # the host table (fp32 torch expressions of warp_by_disp) against a float64 construction
    ref = mc.entries_from_geometry(sc["geom"], sc["edges"], len(sc["edges"]))
    for k in ("depth_row", "flow_row", "image"):
        assert np.array_equal(sc["entries"][k], ref[k])
    scale = max(sc["H"], sc["W"])
    assert np.abs(sc["entries"]["Hm"] - ref["Hm"]).max() <= 16 * 2.0 ** -24 * scale
    assert np.abs(sc["entries"]["Kt"] - ref["Kt"]).max() <= 16 * 2.0 ** -24 * scale
    g, t = sc["geom"], torch.from_numpy
    D_i, D_j = mc.depth_maps(sc)
    masks, means = motion_masks_torch(sc["edges"], sc["N"], t(g["K_i"]), t(g["K_j"]), t(g["pose_i"][:, :3, :3]), t(g["pose_j"][:, :3, :3]),
                                      t(g["pose_i"][:, :3, 3:]), t(g["pose_j"][:, :3, 3:]), t(D_i), t(D_j), t(sc["flow_ij"]),
                                      t(sc["flow_ji"]), mc.THRE)
    differ = mc.check_agreement(torch.stack(masks).numpy(), torch.stack(means).numpy(), mean, mask, flagged, info)
    dev = float(np.abs(torch.stack(means).numpy() - mean).max())
    record_margin(f"motion_cpu_{name}", flagged_share=info["flagged"], masked_share=info["masked"], eps=float(info["eps"].max()),
                  torch_mean_dev=dev, flagged_differing=differ)
    # the moving rectangle is found whole (the upper part of the ramp region is masked too)
    for m in mask:
        assert m[sc["moving"]].all()


def test_chunk_scene_has_min_and_max_in_different_chunks(scenes):
    info = scenes["4x(40x52)"]["oracle"][3]
    assert all(lo // 1024 != hi // 1024 for _, _, lo, hi in info["ranges"])


def test_oracle_nan_and_constant_maps(scenes):
    """One NaN flow value, or an exactly constant error map, turns the entry's contribution into NaN: every image it votes for gets a
    NaN mean and an all-false mask; the other images are as before."""
    sc = scenes["3x(37x41)"]
    H, W, lists = sc["H"], sc["W"], sc["lists"]
    base_mask = sc["oracle"][1]
    fij = sc["flow_ij"].copy()
    fij[0, 1, 5, 7] = np.nan                                         # entry 0 votes for image edges[0][0]
    mean, mask, flagged, info = mc.oracle(sc["entries"], sc["pred_i"], sc["pred_j"], fij, sc["flow_ji"], lists, H, W)
    hit = sc["edges"][0][0]
    assert info["nan_images"] == [hit] and np.isnan(mean[hit]).all() and not mask[hit].any()
    for n in range(sc["N"]):
        if n != hit:
            assert np.array_equal(mask[n], base_mask[n])
    ent, fij, fji = constant_entry(sc, 1)
    mean, mask, flagged, info = mc.oracle(ent, sc["pred_i"], sc["pred_j"], fij, fji, lists, H, W)
    hit = int(ent["image"][1])
    assert info["nan_images"] == [hit] and not mask[hit].any() and info["ranges"][1][:2] == (5.0, 5.0)


def constant_entry(sc, k):
    """(entries, flow_ij, flow_ji) with entry k turned into an exactly constant error map in every arithmetic: H maps every pixel to
    the origin, K t = 0 and the flow is (3 - x, 4 - y), so that err = |(0 - x) - (3 - x), (0 - y) - (4 - y)| = 5 in integers."""
    ent = sc["entries"].copy()
    ent["Hm"][k] = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    ent["Kt"][k] = 0
    fij, fji = sc["flow_ij"].copy(), sc["flow_ji"].copy()
    E = len(sc["edges"])
    row = int(ent["flow_row"][k])
    fl = fij if row < E else fji
    ys, xs = np.meshgrid(np.arange(sc["H"], dtype=np.float32), np.arange(sc["W"], dtype=np.float32), indexing="ij")
    fl[row % E, 0], fl[row % E, 1] = 3 - xs, 4 - ys
    return ent, fij, fji


# ------------------------------------------------------------------------------------------------ files
class _Scene:
    """What the writers read, without an engine."""
    def __init__(self, masks, confs):
        from align3r_amd.dust3r.cloud_opt.commons import get_conf_trf
        self.dynamic_masks, self.init_conf_maps, self.conf_trf = masks, confs, get_conf_trf("log")

    def get_init_conf(self, mode=None):
        from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer
        return PointCloudOptimizer.get_init_conf(self, mode)


def test_mask_png_and_init_conf_writers_round_trip(tmp_path):
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer
    rng = np.random.default_rng(0)
    masks = [torch.from_numpy(rng.random((9, 13)) < 0.3) for _ in range(3)]
    confs = [torch.from_numpy((1 + 4 * rng.random((9, 13))).astype(np.float32)) for _ in range(3)]
    sc = _Scene(masks, confs)
    assert PointCloudOptimizer.save_dynamic_masks(sc, str(tmp_path), 4) is masks
    out = PointCloudOptimizer.save_init_conf_maps(sc, str(tmp_path), start=4)
    for i in range(3):
        im = PIL.Image.open(tmp_path / f"dynamic_mask_{4 + i}.png")
        arr = np.array(im)
        assert im.mode == "L" and arr.dtype == np.uint8 and set(np.unique(arr).tolist()) <= {0, 255}
        assert np.array_equal(arr == 255, masks[i].numpy())
        c = np.load(tmp_path / f"init_conf_{4 + i}.npy")
        assert c.dtype == np.float32 and np.array_equal(c, confs[i].log().numpy()) and np.array_equal(c, out[i].numpy())
    sc.dynamic_masks = None
    with pytest.raises(RuntimeError, match="no dynamic masks"):
        PointCloudOptimizer.save_dynamic_masks(sc, str(tmp_path))


@pytest.mark.parametrize("k", [3, 5])
def test_enlarge_seg_masks(tmp_path, k):
    from align3r_amd.dust3r.utils.image_pose import enlarge_seg_masks
    mask = np.zeros((12, 15), np.uint8)
    mask[6, 7] = 255                      # interior
    mask[0, 0] = 255                      # corner: the window is cut by the border
    mask[11, 3] = 255                     # bottom edge
    PIL.Image.fromarray(mask).save(tmp_path / "dynamic_mask_0.png")
    PIL.Image.fromarray(np.zeros((12, 15), np.uint8)).save(tmp_path / "dynamic_mask_1.png")
    written = enlarge_seg_masks(str(tmp_path), kernel_size=k)
    assert sorted(os.path.basename(w) for w in written) == ["enlarged_dynamic_mask_0.png", "enlarged_dynamic_mask_1.png"]
    want = np.zeros_like(mask)
    r = k // 2
    for y, x in ((6, 7), (0, 0), (11, 3)):
        want[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = 255
    got = np.array(PIL.Image.open(tmp_path / "enlarged_dynamic_mask_0.png"))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert not np.array(PIL.Image.open(tmp_path / "enlarged_dynamic_mask_1.png")).any()
    assert np.array_equal(np.array(PIL.Image.open(tmp_path / "dynamic_mask_0.png")), mask)          # the source stays


def test_run_clip_flow_arguments():
    from align3r_amd.tool import run_clip
    base = ["--images", "x", "--weights", "y", "--out", "z"]
    a = run_clip.parse(base)
    assert a.flow is False and a.scene_graph == "swin-3-noncyclic"
    a = run_clip.parse(base + ["--flow", "--flow-weights", "raft.pth"])
    assert a.flow and a.scene_graph == "swinstride-5-noncyclic" and a.flow_weights == "raft.pth" and a.gt_masks is None
    assert run_clip.parse(base + ["--flow", "--scene-graph", "swin-2"]).scene_graph == "swin-2"
    for bad in (["--flow", "--hierarchical"], ["--flow-weights", "raft.pth"], ["--gt-masks", "m"], ["--not-shared-focal"]):
        with pytest.raises(SystemExit):
            run_clip.parse(base + bad)


def test_refusals_before_any_launch():
    """A graph that is not symmetrised keeps the reference's assert; an image in no pair of the first half and mixed shapes raise."""
    from align3r_amd.dust3r.cloud_opt_flow.optimizer import PointCloudOptimizer

    class Bare:
        get_motion_mask_from_pairs = PointCloudOptimizer.get_motion_mask_from_pairs
        motion_mask_thre = 0.35

    b = Bare()
    z = torch.zeros(4, 2, 4, 6)
    b.is_symmetrized, b.edges, b.n_imgs, b.imshape, b._uniform = False, [(0, 1), (1, 2)], 3, (4, 6), True
    with pytest.raises(AssertionError, match="only support symmetric case"):
        b.get_motion_mask_from_pairs(None, None, None, None, z, z)
    b.is_symmetrized, b.edges = True, [(0, 1), (1, 2), (1, 0), (2, 1)]
    b._uniform = False
    with pytest.raises(RuntimeError, match="one shape"):
        b.get_motion_mask_from_pairs(None, None, None, None, z, z)
    b._uniform, b.edges = True, [(0, 1), (1, 0), (1, 2), (2, 1)]                 # image 2 is in no pair of the first half
    with pytest.raises(RuntimeError, match=r"images \[2\]"):
        b.get_motion_mask_from_pairs(None, None, None, None, z, z)


def test_c_call_validates_on_the_host_before_any_launch():
    """a3r_motion_masks refuses bad arguments from the host copies of its tables, before it touches the device: no GPU is needed."""
    import ctypes as C
    from align3r_amd import _lib
    lib = _lib.load()
    N, graph, H, W, kw = mc.SCENES["3x(37x41)"]
    sc = mc.make_scene(N, graph, H, W, **kw)
    entries = np.ascontiguousarray(_entries(sc))
    E, M = len(sc["edges"]), len(sc["edges"]) // 2
    start = np.zeros(N + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in sc["lists"]])
    flat = np.asarray([k for l in sc["lists"] for k in l], np.int32)
    need = int(lib.a3r_motion_workspace_bytes(M, N, H * W))
    assert need >= 2 * M * H * W * 4 and lib.a3r_motion_workspace_bytes(0, N, H * W) == 0
    fake = 1 << 20                                            # stands for a device pointer: never dereferenced on these paths

    def call(ws=fake, ws_bytes=need, masks=fake, **over):
        f = dict(M=M, N=N, E=E, H=H, W=W, motion_mask_thre=0.35, pred_i=fake, pred_j=fake, flow_ij=fake, flow_ji=fake, entries=fake,
                 entries_host=entries.ctypes.data, list_start=fake, list_start_host=start.ctypes.data, list_entry=fake,
                 list_entry_host=flat.ctypes.data)
        f.update(over)
        rc = lib.a3r_motion_masks(C.byref(_lib.MotionDesc(**f)), ws, ws_bytes, masks, None, None)
        return rc, lib.a3r_last_error().decode()

    for kw_, msg in ((dict(M=0), "must be positive"), (dict(W=-3), "must be positive"), (dict(flow_ij=None), "null pointmap or flow"),
                     (dict(list_entry_host=None), "null entry table"), (dict(masks=None), "null mask"), (dict(ws=None), "workspace too small"),
                     (dict(ws_bytes=need - 1), "workspace too small"), (dict(ws=fake + 8), "16-byte aligned"),
                     (dict(motion_mask_thre=float("nan")), "NaN")):
        rc, err = call(**kw_)
        assert rc == -1 and msg in err, (kw_, err)
    for field, value in (("depth_row", 2 * E), ("flow_row", -1), ("image", N)):
        keep = entries[field][1]
        entries[field][1] = value
        rc, err = call()
        entries[field][1] = keep
        assert rc == -1 and field in err, (field, err)
    flat[0] = 2 * M
    rc, err = call()
    flat[0] = 0
    assert rc == -1 and "list entry" in err
    start[1] = 0
    rc, err = call()
    assert rc == -1 and "empty list" in err
