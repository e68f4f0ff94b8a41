"""Writes compaction_parent.json: what the entries built on the count / scan / place compaction compute (csrc/scene.hip point cloud
and mesh, voxel.hip, match.hip, tsdf.hip surface, metrics.hip 'scale' rule), as the library selected by A3R_LIB (default: the
tree's own) computes it on the GPU.  The committed file pins the results of the commit BEFORE the workgroup rank, the scan kernel
and the host epilogue were shared (csrc/compact.h):

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_compaction_parent.py [--out FILE]

A case is one (entry family, shape or size); its record maps every call of the case to the SHA-256 of the raw bytes of all of the
call's outputs.  Ranks, offsets and hash-table winners are integers and the float outputs are written once each from per-item
arithmetic, so a record is the same in every run.

  scene/<kind>/<shape>   an AlignEngine over a problem of tests/align_cases.py, parameters as drawn (never iterated); kind plain | mono;
                         shapes 2x3, 37x41 (scalar loads, ragged second chunk), 32x32 (P = one chunk), 36x44 (vector loads, two
                         chunks), mixed = 32x48 with 24x40 (padding).  Masks all | none | one | half; per mask export_points
                         (xyz, index, rgb), count_points (per-image counts) and export_mesh single- and double-sided (xyz, rgb,
                         faces, face_rgb)
  voxel/<M>              voxel_downsample, best and mean, with and without rgb + priority; M = 1, 63, 1024, 1025 and 1024 * 1024 +
                         1025 (1026 chunks: a scan thread owns two counts)
  match/<n2>             reciprocal_matches against n1 = 1, 7, 1000 for n2 = 1, 65, 1024, 1025; n1 = 3 for n2 = 1024 * 1024 + 1025
                         (pairs, flags, both index arrays)
  tsdf/<name>            tsdf_integrate + tsdf_mesh of the cases of tests/tsdf_cases.py that have a surface and of gates-1x8x8 (no
                         cell); tsdf/nvox1025 = tsdf_mesh of a synthetic 5 x 5 x 41 grid (vertices, colours, faces)
  depth/<n>              depth_align(mode='scale') and depth_metrics on n = 1, 63, 1024, 1025, 5000 elements, about half valid
                         (scale and shift, the info block, the metrics)

tests/test_gpu_compaction_parent.py imports CASES and measure_case() from here, so the test and the golden cannot drift apart."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import align_cases as ac        # noqa: E402
import tsdf_cases as tc         # noqa: E402

BIG = 1024 * 1024 + 1025        # 1026 chunks of 1024 items: more chunks than the scan has threads
SCENE_SHAPES = {"2x3": (2, 3), "37x41": (37, 41), "32x32": (32, 32), "36x44": (36, 44), "mixed": (32, 48)}
MIXED = [(32, 48), (24, 40), (32, 48), (24, 40)]
VOXEL_M = (1, 63, 1024, 1025, BIG)
MATCH_N2 = {1: (1, 7, 1000), 65: (1, 7, 1000), 1024: (1, 7, 1000), 1025: (1, 7, 1000), BIG: (3,)}
TSDF_NAMES = ("plane", "sphere", "sphere-noisy", "ragged-70x65x40", "gates-1x8x8", "nvox1025")
DEPTH_N = (1, 63, 1024, 1025, 5000)

CASES = {}
for _kind in ("plain", "mono"):
    for _tag in SCENE_SHAPES:
        CASES[f"scene/{_kind}/{_tag}"] = dict(family="scene", kind=_kind, tag=_tag)
for _m in VOXEL_M:
    CASES[f"voxel/{_m}"] = dict(family="voxel", M=_m)
for _n2 in MATCH_N2:
    CASES[f"match/{_n2}"] = dict(family="match", n2=_n2)
for _name in TSDF_NAMES:
    CASES[f"tsdf/{_name}"] = dict(family="tsdf", name=_name)
for _n in DEPTH_N:
    CASES[f"depth/{_n}"] = dict(family="depth", n=_n)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"<none>")
        elif isinstance(t, int):
            h.update(str(t).encode())
        else:
            h.update(repr(tuple(t.shape)).encode())
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------- scene
def _engine(kind, tag):
    from align3r_amd.aligner import AlignEngine
    mixed = tag == "mixed"
    H, W = SCENE_SHAPES[tag]
    N = 4 if mixed else 3
    prob = ac.flow_problem(N, H, W, ac.window_graph(N, 2), 21, dyn_frac=0.3, pxl_thre=1e9, thre=1e9, shared_focal=False, train_pp=False,
                           full_dynamic=False, guard=False)
    args = list(prob["args"])
    if mixed:
        args[6] = MIXED                 # the small images use the first 960 of the P = 1536 entries of their rows
    rng = np.random.default_rng(77)
    mono = (1 + rng.random((N, H * W))).astype(np.float32) if kind == "mono" else None
    eng = AlignEngine(*args, mono=mono, device="cuda:0")
    init = dict(prob["init"])
    if kind == "mono":
        init["shifts"] = (0.05 * rng.standard_normal(N)).astype(np.float32)
    eng.set_params(**init)
    return eng, rng


def _scene(case):
    eng, rng = _engine(case["kind"], case["tag"])
    N, P = eng.N, eng.P
    conf = (1 + 9 * rng.random((N, P))).astype(np.float32)
    rgb = rng.integers(0, 256, (N, P, 3), dtype=np.uint8)
    one = np.ones((N, P), bool)
    one[1, int(eng.imarea[1]) // 2] = False
    masks = dict(all=(0.0, None), none=(11.0, None), one=(0.0, one), half=(2.0, rng.random((N, P)) < 0.45))
    rec = {}
    for tag, (thr, dyn) in masks.items():
        pts = eng.export_points(conf, thr, dyn=dyn, rgb=rgb, with_index=True)
        rec[f"{tag}/points"] = _sha(pts["xyz"], pts["index"], pts["rgb"])
        total, per_img = eng.count_points(conf, thr, dyn=dyn)
        rec[f"{tag}/counts"] = _sha(total, per_img)
        for ds in (False, True):
            m = eng.export_mesh(conf, thr, dyn=dyn, rgb=rgb, double_sided=ds)
            rec[f"{tag}/mesh{2 if ds else 1}"] = _sha(m["xyz"], m["rgb"], m["faces"], m["face_rgb"])
    return rec


# ------------------------------------------------------------------------------------------------- voxel
def _voxel(case):
    from align3r_amd import ops
    M = case["M"]
    rng = np.random.default_rng(1000 + M % 9973)
    xyz = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    if M > 8:
        xyz[rng.integers(0, M, max(M // 50, 1))] = np.nan           # points in no voxel
    prio = rng.integers(0, 4, M).astype(np.float32)                 # few levels: ties go to the lowest row
    rgb = rng.integers(0, 256, (M, 3), dtype=np.uint8)
    xyz, prio, rgb = _dev(xyz), _dev(prio), _dev(rgb)
    rec = {}
    for reduce in ("best", "mean"):
        for full in (False, True):
            out = ops.voxel_downsample(xyz, 0.05, priority=prio if full else None, rgb=rgb if full else None, reduce=reduce,
                                       min_count=2 if M > 4096 else 1)
            rec[f"{reduce}/{'rgb_prio' if full else 'bare'}"] = _sha(out["xyz"], out.get("rgb"), out["index"], out["count"], out["dropped"])
    return rec


# ------------------------------------------------------------------------------------------------- matches
def _match(case):
    from align3r_amd import ops
    n2 = case["n2"]
    rec = {}
    for n1 in MATCH_N2[n2]:
        rng = np.random.default_rng(7 * n1 + n2 % 9973)
        p1 = rng.standard_normal((n1, 3)).astype(np.float32)
        p2 = (p1[rng.integers(0, n1, n2)] + 0.05 * rng.standard_normal((n2, 3))).astype(np.float32)
        out = ops.reciprocal_matches(_dev(p1), _dev(p2))
        rec[f"n1={n1}"] = _sha(out["pairs"], out["reciprocal_in_P2"].view(_torch().uint8), out["nn2_in_P1"], out["nn1_in_P2"], out["count"])
    return rec


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------- TSDF surface
def _tsdf(case):
    from align3r_amd import ops
    name = case["name"]
    if name == "nvox1025":
        nx, ny, nz = 5, 5, 41
        rng = np.random.default_rng(3)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        tsdf = np.clip((k - 20.3 + 3.0 * np.sin(0.9 * i) * np.cos(0.7 * j)) / 4.0, -1, 1).astype(np.float32)
        wsum = (rng.random((nz, ny, nx)) < 0.9).astype(np.float32)
        rgb = rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
        grid, origin, voxel, min_weight = (_dev(tsdf), _dev(wsum), _dev(rgb)), (0.1, -0.2, 0.3), 0.05, 0.5
    else:
        c = tc.build(name)
        grid = ops.tsdf_integrate(_dev(c["depth"]), _dev(c["weight"]), _dev(c["rgb"]), c["cams"], c["origin"], c["dims"], c["voxel"],
                                  c["trunc"], near=c["near"], max_depth=c["max_depth"])
        origin, voxel, min_weight = c["origin"], c["voxel"], c["min_weight"]
    xyz, colours, faces = ops.tsdf_mesh(grid[0], grid[1], grid[2], origin, voxel, min_weight)
    bare = ops.tsdf_mesh(grid[0], grid[1], None, origin, voxel, min_weight)
    return {"mesh": _sha(xyz, colours, faces), "mesh/no_rgb": _sha(bare[0], bare[2])}


# ------------------------------------------------------------------------------------------------- depth evaluation
def _depth(case):
    from align3r_amd import ops
    n = case["n"]
    rng = np.random.default_rng(50 + n)
    gt = rng.uniform(0.5, 60.0, n).astype(np.float32)
    pred = (gt.astype(np.float64) / 2.5 * np.exp(0.05 * rng.standard_normal(n))).astype(np.float32)
    if n > 1:
        gt[rng.random(n) < 0.5] = 0.0                               # about half of the elements are not valid
    pred, gt = _dev(pred), _dev(gt)
    st, info = ops.depth_align(pred, gt, 70.0, "scale")
    return {"scale": _sha(st, info), "metrics": _sha(ops.depth_metrics(pred, gt, 70.0, st))}


_FAMILIES = dict(scene=_scene, voxel=_voxel, match=_match, tsdf=_tsdf, depth=_depth)


def measure_case(name):
    """the record of one case from the loaded library"""
    case = CASES[name]
    return _FAMILIES[case["family"]](case)


if __name__ == "__main__":
    import time
    dst = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(HERE, "compaction_parent.json")
    records = {}
    for name in CASES:
        t0 = time.time()
        records[name] = measure_case(name)
        print(name, "ok", len(records[name]), f"{time.time() - t0:.2f} s", flush=True)
    with open(dst, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(records)} cases to {dst}")
