"""GPU: clean_pointcloud on the aligner handle (csrc/scene.hip: a3r_align_scene_clean) against the float64 oracle of
tests/clean_cases.py, under its agreement rule: bit-equal on the pixels no rounding error can move, the original or the clipped
value on the flagged ones, padding bit-untouched.  The oracle reads the state back through the scene's own getters after the fact
(get_depthmaps(raw), get_focals, get_principal_points, get_im_poses), as tests/test_gpu_scene.py does.  Flagged and changed shares
are recorded as clean_<case>.
Shapes: 2x3 (fewer pixels than a wave), 37x41 (P % 4 != 0: scalar form, ragged last chunk), 36x44 (vector form, two chunks),
32x48 mixed with 24x40 (padding), the mono form with shifts, the flow class with a shared focal.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clean_cases as cc
from conftest import record_margin
from test_gpu_scene import make_mixed_scene, make_scene, _problem

pytestmark = pytest.mark.gpu

A3R_EINVAL = -1
PAD = 7.25                   # confidence written at the padding entries: above every real one, so a padding pixel taken for visible shows

CASES = {                    # name: (kind, scene of clean_cases.SCENES)
    "plain_2x3": ("plain", "3x(2x3)"),
    "plain_37x41": ("plain", "5x(37x41)"),
    "plain_36x44": ("plain", "4x(36x44)"),
    "mixed_32x48_24x40": ("mixed", "mixed"),
    "mono_36x44": ("mono", "4x(36x44)"),
    "flow_sf_37x41": ("flow", "5x(37x41)"),
}


def build(name):
    """(scene with the helper scene as its state and its confidences as im_conf, the helper scene)"""
    kind, key = CASES[name]
    shapes, kw = cc.SCENES[key]
    sc = cc.make_scene(shapes, shared_focal=(kind == "flow"), **kw)
    if kind == "mixed":
        scene, _ = make_mixed_scene()
    else:
        scene, _ = make_scene(kind, len(shapes), *shapes[0])
    assert [tuple(s) for s in scene.imshapes] == [tuple(s) for s in shapes]
    if kind == "mono":
        shifts = 0.05 * np.asarray([1.0, -2.0, 3.0, -1.0])[:len(shapes)]
        par = cc.engine_params(sc, mono=scene.engine.mono.cpu().numpy(), shifts=shifts)
    else:
        par = cc.engine_params(sc)
    scene.engine.set_params(**par)
    scene.im_conf = [torch.from_numpy(c.copy()) for c in sc["conf"]]
    return scene, sc


def state_np(scene):
    """(depth maps, c2w, focals, principal points) of the scene's current state, from its getters"""
    host = lambda t: t.detach().cpu().numpy()
    return (cc.unstack(host(scene.get_depthmaps(raw=True)), scene.imshapes), host(scene.get_im_poses()),
            host(scene.get_focals()).reshape(-1), host(scene.get_principal_points()))


def run_and_check(name, scene, conf_maps, tol=0.001, bad_conf=0.0, cap=True, tag=""):
    """engine.clean_confidences on the stacked maps against the oracle; returns (got [N,P], oracle out, flagged, info)."""
    shapes, P = scene.imshapes, scene.max_area
    conf = cc.stack(conf_maps, shapes, P, fill=PAD)
    got = scene.engine.clean_confidences(torch.from_numpy(conf), tol=tol, bad_conf=bad_conf).cpu().numpy()
    depth, c2w, f, pp = state_np(scene)
    out, flagged, info = cc.oracle(depth, c2w, f, pp, conf_maps, shapes, tol=tol, bad_conf=bad_conf)
    differ = cc.check_agreement(cc.unstack(got, shapes), conf_maps, out, flagged, bad_conf=bad_conf)
    for n, (h, w) in enumerate(shapes):                                   # padding: bit-untouched
        assert np.array_equal(got[n, h * w:].view(np.uint32), conf[n, h * w:].view(np.uint32)), n
    record_margin(f"clean_{name}{tag}", flagged_share=info["flagged"], changed_share=info["changed"], eps_px=info["eps_px"],
                  flagged_differing=differ, pixels=info["pixels"])
    if cap:
        cc.assert_cap(info)
    return got, out, flagged, info


@pytest.mark.parametrize("name", list(CASES))
def test_engine_vs_oracle(name):
    scene, sc = build(name)
    got, out, _, info = run_and_check(name, scene, sc["conf"])
    conf = cc.stack(sc["conf"], scene.imshapes, scene.max_area, fill=PAD)
    assert (got.view(np.uint32) != conf.view(np.uint32)).sum() >= 1        # the kernel did clip something
    assert set(np.unique(got[got != conf]).tolist()) <= {0.0}


def test_images_are_processed_in_order():
    """Image i reads the FINISHED rows below it: on this scene an oracle in which every image reads the original confidences
    differs from the sequential one on unflagged pixels, and the kernel matches the sequential one."""
    scene, sc = build("plain_36x44")
    got, seq, flagged, _ = run_and_check("plain_36x44", scene, sc["conf"], tag="_order")
    depth, c2w, f, pp = state_np(scene)
    par, _, _ = cc.oracle(depth, c2w, f, pp, sc["conf"], scene.imshapes, sequential=False)
    differ = [(a != b) & ~m for a, b, m in zip(seq, par, flagged)]
    assert sum(int(d.sum()) for d in differ) > 0                           # the scene discriminates
    for g, s, d in zip(cc.unstack(got, scene.imshapes), seq, differ):
        assert np.array_equal(g[d], s[d])


@pytest.mark.parametrize("tol", [0.0, 0.05])
def test_tol_and_bad_conf(tol):
    scene, sc = build("plain_37x41")
    got, out, _, info = run_and_check("plain_37x41", scene, sc["conf"], tol=tol, bad_conf=2.0, tag=f"_tol{tol}_bad2")
    conf = cc.stack(sc["conf"], scene.imshapes, scene.max_area, fill=PAD)
    low = conf <= 2.0
    assert low.sum() > 100 and np.array_equal(got[low], conf[low])         # already below bad_conf: as they were
    moved = got != conf
    assert moved.sum() > 0 and (got[moved] == 2.0).all() and (conf[moved] > 2.0).all()


def test_nan_confidences_nonfinite_depth_and_guard_rows():
    """NaN confidences survive and never clip anything, a depth of +inf is no fault, and the call writes nothing outside [N,P]:
    the buffer sits between two guard rows, the workspace in front of guard bytes."""
    from align3r_amd._lib import check, ptr, stream_ptr
    scene, sc = build("plain_36x44")
    eng, lib, dev = scene.engine, scene.engine.lib, scene.engine.device
    N, P = eng.N, eng.P
    depth = eng.params["depth"].clone()
    depth[1, 700] = 100.0                                                  # exp overflows: depth +inf, the pixel's point is not finite
    eng.set_params(depth=depth, reset_optimizer=False)
    conf_maps = [c.copy() for c in sc["conf"]]
    rng = np.random.default_rng(0)
    for n in range(N):
        idx = rng.choice(P, 40, replace=False)
        conf_maps[n].reshape(-1)[idx] = np.nan
    conf = cc.stack(conf_maps, scene.imshapes, P)
    depth_np, c2w, f, pp = state_np(scene)
    assert np.isinf(depth_np[1].reshape(-1)[700])
    out, flagged, info = cc.oracle(depth_np, c2w, f, pp, conf_maps, scene.imshapes)
    cc.assert_cap(info)
    GUARD = -12345.5
    buf = torch.full((N + 2, P), GUARD, device=dev)
    buf[1:N + 1] = torch.from_numpy(conf).to(dev)
    need = int(lib.a3r_align_scene_clean_workspace_bytes(N, P))
    ws = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)
    check(lib.a3r_align_scene_clean(eng.handle, buf[1].data_ptr(), 0.001, 0.0, ptr(ws), need, stream_ptr()), "a3r_align_scene_clean")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[0] == GUARD).all() and (got[N + 1] == GUARD).all() and (ws[need:] == 0xAB).all()
    got = got[1:N + 1]
    assert np.array_equal(np.isnan(got), np.isnan(conf)) and np.isnan(conf).sum() == 40 * N
    cc.check_agreement(cc.unstack(got, scene.imshapes), conf_maps, out, flagged)
    assert (got != conf)[~np.isnan(conf)].sum() > 0
    record_margin("clean_plain_36x44_nan_inf", flagged_share=info["flagged"], changed_share=info["changed"])


def test_deterministic_and_edge_shard_handle_equal_to_fused():
    from align3r_amd.aligner import AlignEngine, ShardedAlignEngine
    shapes, kw = cc.SCENES["4x(36x44)"]
    sc = cc.make_scene(shapes, **kw)
    prob = _problem(len(shapes), *shapes[0], 11)
    par = dict(cc.engine_params(sc), pw_poses=prob["init"]["pw_poses"])
    conf = cc.stack(sc["conf"], shapes)
    fused = AlignEngine(*prob["args"], device="cuda:0")
    fused.set_params(**par)
    a, b = fused.clean_confidences(conf), fused.clean_confidences(conf)
    assert torch.equal(a, b) and (a.cpu().numpy() != conf).sum() > 0
    shard = ShardedAlignEngine(*prob["args"], device="cuda:0", local_shards=2)
    shard.set_params(**par)
    c = shard.clean_confidences(conf)
    assert torch.equal(a, c)


def test_bad_arguments_are_refused_before_anything_is_written():
    from align3r_amd._lib import ptr, stream_ptr
    scene, sc = build("plain_36x44")
    eng, lib, dev = scene.engine, scene.engine.lib, scene.engine.device
    N, P = eng.N, eng.P
    conf = torch.from_numpy(cc.stack(sc["conf"], scene.imshapes, P)).to(dev)
    keep = conf.clone()
    need = int(lib.a3r_align_scene_clean_workspace_bytes(N, P))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    call = lambda c, tol, bad, w, nbytes: lib.a3r_align_scene_clean(eng.handle, c, tol, bad, w, nbytes, stream_ptr())
    for args, msg in (((None, 0.001, 0.0, ptr(ws), need), "null confidence"),
                      ((ptr(conf), 0.001, 0.0, ptr(ws), need - 1), "workspace too small"),
                      ((ptr(conf), 0.001, 0.0, None, need), "workspace too small"),
                      ((ptr(conf), 0.001, 0.0, ws.data_ptr() + 4, need), "16-byte aligned"),
                      ((ptr(conf), 1.0, 0.0, ptr(ws), need), "tol"),
                      ((ptr(conf), -0.1, 0.0, ptr(ws), need), "tol"),
                      ((ptr(conf), float("nan"), 0.0, ptr(ws), need), "tol"),
                      ((ptr(conf), 0.001, float("nan"), ptr(ws), need), "bad_conf")):
        assert call(*args) == A3R_EINVAL, msg
        assert msg in lib.a3r_last_error().decode(), (msg, lib.a3r_last_error())
        torch.cuda.synchronize()
        assert torch.equal(conf, keep), msg
    with pytest.raises(RuntimeError, match="tol"):
        eng.clean_confidences(conf, tol=1.0)
    assert call(ptr(conf), 0.001, 0.0, ptr(ws), need) == 0                  # and the same buffers are accepted
    torch.cuda.synchronize()
    assert not torch.equal(conf, keep)


def test_scene_method_device_and_torch_paths(monkeypatch):
    from align3r_amd.dust3r.cloud_opt.init_im_poses import inv_rigid
    from align3r_amd.dust3r.cloud_opt.optimizer import clean_pointcloud
    monkeypatch.delenv("A3R_CLEAN", raising=False)
    scene, sc = build("plain_36x44")
    shapes, P = scene.imshapes, scene.max_area
    depth, c2w, f, pp = state_np(scene)
    out, flagged, info = cc.oracle(depth, c2w, f, pp, sc["conf"], shapes)
    want = scene.engine.clean_confidences(cc.stack(sc["conf"], shapes, P)).cpu().numpy()
    kinds = [(c.device, c.dtype) for c in scene.im_conf]
    assert scene.clean_pointcloud() is scene
    assert [(c.device, c.dtype) for c in scene.im_conf] == kinds and [tuple(c.shape) for c in scene.im_conf] == [tuple(s) for s in shapes]
    dev_maps = [c.cpu().numpy() for c in scene.im_conf]
    assert np.array_equal(cc.stack(dev_maps, shapes, P).view(np.uint32), want.view(np.uint32))
    # a following export keeps exactly get_masks()
    pc = scene.get_pointcloud(with_index=True)
    masks = torch.nonzero(torch.cat([m.flatten() for m in scene.get_masks()])).flatten().cpu().numpy()
    assert 0 < len(masks) < scene.n_imgs * P and np.array_equal(pc["index"].cpu().numpy(), masks)
    # A3R_CLEAN=torch: the module function, bit for bit
    scene2, _ = build("plain_36x44")
    ref = clean_pointcloud([c.to(scene2.device) for c in scene2.im_conf], scene2.get_intrinsics(), inv_rigid(scene2.get_im_poses()),
                           scene2.get_depthmaps(), scene2.get_pts3d(), tol=0.001, bad_conf=0)
    monkeypatch.setenv("A3R_CLEAN", "torch")
    assert scene2.clean_pointcloud() is scene2
    torch_maps = [c.cpu().numpy() for c in scene2.im_conf]
    for a, b in zip(torch_maps, ref):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    # both paths under the agreement rule
    d_dev = cc.check_agreement(dev_maps, sc["conf"], out, flagged)
    d_torch = cc.check_agreement(torch_maps, sc["conf"], out, flagged)
    differ = sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(dev_maps, torch_maps))
    record_margin("clean_scene_method_36x44", flagged_share=info["flagged"], changed_share=info["changed"], device_vs_oracle_flagged=d_dev,
                  torch_vs_oracle_flagged=d_torch, device_vs_torch_pixels=differ)
    assert sum(int((a != b).sum()) for a, b in zip(torch_maps, sc["conf"])) > 0


def test_hierarchical_driver_cleans_when_asked(monkeypatch, tmp_path):
    """The synthetic clip of tests/test_gpu_hier.py through hierarchical_alignment with and without clean=True: every written
    confidence map is at most what the plain run wrote, and some are lower."""
    import align3r_amd.dust3r.inference as inf_mod
    from align3r_amd.tool import hierarchical as hz
    from align3r_amd.tool import run_clip
    from test_gpu_hier import _scene
    monkeypatch.delenv("A3R_CLEAN", raising=False)
    N, H, W = 8, 32, 48
    cams, world, f = _scene(N, H, W)
    imgs = [dict(idx=i, instance=str(i), true_shape=np.int32([[H, W]])) for i in range(N)]

    def run(clean, out_dir):
        rng = np.random.default_rng(0)

        def fake_inference(pairs, model, device, batch_size=1, verbose=False):
            gi = [int(a["instance"]) for a, b in pairs]
            gj = [int(b["instance"]) for a, b in pairs]
            p1 = np.stack([0.7 * ((world[i] - cams[i][1]) @ cams[i][0]) for i in gi]).astype(np.float32)
            p2 = np.stack([0.7 * ((world[j] - cams[i][1]) @ cams[i][0]) for i, j in zip(gi, gj)]).astype(np.float32)
            c = (2 + 8 * rng.random((len(pairs), H, W))).astype(np.float32)
            return dict(view1=dict(idx=[a["idx"] for a, b in pairs]), view2=dict(idx=[b["idx"] for a, b in pairs]),
                        pred1=dict(pts3d=torch.from_numpy(p1), conf=torch.from_numpy(c)),
                        pred2=dict(pts3d_in_other_view=torch.from_numpy(p2), conf=torch.from_numpy(c.copy())))

        monkeypatch.setattr(inf_mod, "inference", fake_inference)
        torch.manual_seed(0)
        kw = dict(clean=True) if clean else {}
        hz.hierarchical_alignment(imgs, None, "cuda", clip_size=3, niter=10, schedule="linear", lr=0.01, min_conf_thr=1.5,
                                  clamp_conf=False, output_dir=str(out_dir), **kw)
        return [np.load(out_dir / f"conf_{i}.npy") for i in range(N)]

    plain, cleaned = run(False, tmp_path / "plain"), run(True, tmp_path / "clean")
    lower = 0
    for a, b in zip(plain, cleaned):
        assert a.shape == b.shape == (H, W) and (b <= a).all()
        lower += int((b < a).sum())
    record_margin("clean_hier_driver", lowered_share=lower / (N * H * W))
    assert lower >= 1
    base = ["--images", "x", "--weights", "y", "--out", "z"]
    assert run_clip.parse(base + ["--clean"]).clean is True and run_clip.parse(base).clean is False
