"""CPU (no GPU): the clean_pointcloud oracle of tests/clean_cases.py against the reference's recorded output and against the
reference-pinned torch function; the C ABI of the device path is declared, exported and bound."""
import json
import os
import re

import numpy as np
import pytest
import torch

import clean_cases as cc
from conftest import GOLDEN, REPO


def _torch_clean(sc, pts, tol=0.001, bad_conf=0):
    from align3r_amd.dust3r.cloud_opt.optimizer import clean_pointcloud
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    cams = torch.linalg.inv(t32(sc["c2w"]))
    out = clean_pointcloud([t32(c) for c in sc["conf"]], t32(sc["K"]), cams, [t32(d) for d in sc["depth"]],
                           [t32(p).reshape(h, w, 3) for p, (h, w) in zip(pts, sc["shapes"])], tol=tol, bad_conf=bad_conf)
    return [o.numpy() for o in out]


def test_oracle_reproduces_the_reference_fixture():
    c = json.load(open(os.path.join(GOLDEN, "hier.json")))["clean"]
    f32 = lambda a: np.asarray(a, np.float32)
    K, c2w = f32(c["K"]), f32(c["c2w"])
    conf, depth, want = [f32(x) for x in c["conf"]], [f32(x) for x in c["depth"]], [f32(x) for x in c["out"]]
    shapes = [x.shape for x in conf]
    out, flagged, info = cc.oracle(depth, c2w, K[:, 0, 0], K[:, :2, 2], conf, shapes, tol=0.001, pts=[f32(p) for p in c["pts"]])
    print("hier.json clean:", info)
    cc.assert_cap(info)
    cc.check_agreement(want, conf, out, flagged)


@pytest.mark.parametrize("name", list(cc.SCENES))
@pytest.mark.parametrize("seed_shift", [0, 10, 20])
def test_oracle_agrees_with_the_torch_function(name, seed_shift):
    shapes, kw = cc.SCENES[name]
    kw = dict(kw, seed=kw["seed"] + seed_shift) if seed_shift else kw
    sc = cc.make_scene(shapes, **kw)
    pts = [p.astype(np.float32) for p in cc.world_points(sc["depth"], sc["c2w"], sc["f"], sc["pp"], shapes)]
    for tol, bad in ((0.001, 0.0), (0.05, 2.0)):
        out, flagged, info = cc.oracle(sc["depth"], sc["c2w"], sc["f"], sc["pp"], sc["conf"], shapes, tol=tol, bad_conf=bad, pts=pts)
        print(name, kw["seed"], tol, bad, info)
        if seed_shift == 0 and bad == 0.0:        # the scenes the GPU tests use; other seeds of a 2x3 image may change nothing
            cc.assert_cap(info)
        else:
            assert info["flagged"] <= cc.MAX_FLAGGED
        got = _torch_clean(sc, pts, tol=tol, bad_conf=bad)
        cc.check_agreement(got, sc["conf"], out, flagged, bad_conf=bad)


def test_order_matters_in_the_oracle():
    """The scene of the GPU order test: reading original confidences everywhere gives another result than image after image."""
    shapes, kw = cc.SCENES["4x(36x44)"]
    sc = cc.make_scene(shapes, **kw)
    seq, flagged, _ = cc.oracle(sc["depth"], sc["c2w"], sc["f"], sc["pp"], sc["conf"], shapes)
    par, _, _ = cc.oracle(sc["depth"], sc["c2w"], sc["f"], sc["pp"], sc["conf"], shapes, sequential=False)
    assert sum(int(((a != b) & ~m).sum()) for a, b, m in zip(seq, par, flagged)) > 0


def test_engine_params_decode_to_the_scene():
    import align_cases as ac
    shapes, kw = cc.SCENES["mixed"]
    sc = cc.make_scene(shapes, **kw)
    par = cc.engine_params(sc)
    assert np.abs(ac._pose_rt(par["im_poses"]) - sc["c2w"][:, :3]).max() < 1e-6
    assert np.abs(np.exp(par["im_focals"] / cc.FOCAL_BREAK) / sc["f"] - 1).max() < 1e-5
    pp0 = np.asarray([(w / 2, h / 2) for h, w in shapes], np.float32)
    assert np.abs(pp0 + 10 * par["im_pp"] - sc["pp"]).max() < 1e-5
    assert np.abs(np.exp(par["depth"]) - cc.stack(sc["depth"], shapes, fill=1.0)).max() < 1e-5


def test_clean_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from align3r_amd import _lib
    names = ("a3r_align_scene_clean_workspace_bytes", "a3r_align_scene_clean")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "a3r.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    size = lib.a3r_align_scene_clean_workspace_bytes
    assert size(0, 10) == 0 and size(4, 0) == 0
    assert size(4, 1584) >= 4 * 1584 * 4 + 4 * 17 * 4 and size(4, 1584) % 16 == 0
    assert size(128, 196608) >= 128 * 196608 * 4
    # argument validation comes before the handle is looked at
    for args, msg in (((None, None, 0.001, 0.0, None, 0, None), b"null confidence"),
                      ((None, C.c_void_p(16), 1.0, 0.0, None, 0, None), b"tol"),
                      ((None, C.c_void_p(16), float("nan"), 0.0, None, 0, None), b"tol"),
                      ((None, C.c_void_p(16), 0.0, float("nan"), None, 0, None), b"bad_conf"),
                      ((None, C.c_void_p(16), 0.0, 0.0, None, 0, None), b"null handle")):
        assert lib.a3r_align_scene_clean(*args) != 0
        assert msg in lib.a3r_last_error(), (msg, lib.a3r_last_error())
