"""Scenes, oracle and agreement rule for the clean_pointcloud tests (tests/test_clean_cpu.py, tests/test_gpu_clean.py).  numpy only.

Scenes.  N pinhole views on a shallow arc look at a wavy surface d = 3 + 0.5 sin(x / 3 + n); a share of the pixels is pulled 1.5 in
front of it (floaters), confidences are uniform in [1, 6], every image has its own focal and principal point (the recipe of the
`clean` fixture of tests/golden/hier.json, with per-image intrinsics).  `engine_params` gives the same scene in the aligner's
encodings: depth = log d (or the scale map of the mono form), im_poses = [unit quaternion, signed_log1p(t)], im_focals =
focal_break * log f, im_pp = (pp - (W / 2, H / 2)) / 10.

Oracle.  `oracle` restates cloud_opt/base_opt.py:468-503 in float64 on the fp32-rounded inputs, image after image, and FLAGS every
pixel whose outcome a rounding error of the fp32 implementations could change.  For a pixel (i, p) with conf > bad_conf and a view j:
  * unsure(j): |z| <= BOUND * max|xyz| (the visibility test z > 0), or u or v within eps_px of a half-integer (the rounded target
    pixel; the image borders -0.5 and W - 0.5 are half-integers too);
  * otherwise, if visible: may(j) = z < (1 - tol) d_j (1 + eps_rel) and c_i < c_j (1 + eps_rel); sure(j) = the same with (1 - eps_rel)
    and a target pixel that is not flagged itself (only j < i matters: the rows above i are read as given).
The pixel is flagged when some view is unsure or may fire while no view fires for sure; a pixel some view clips for sure is clipped
whatever the others decide.  eps_px = 2 f_max BOUND max|xyz| / z_min and eps_rel = 10 BOUND follow from the project's bound for aligner
points, BOUND = 1e-5 of max |xyz|: a point error of BOUND max|xyz| moves a projection by f / z times that, twice for x and z.

Agreement rule (`check_agreement`): bit-equal to the oracle on unflagged pixels; the original value or min(original, bad_conf) on
flagged ones; padding entries bit-untouched.
"""
import numpy as np

BOUND = 1e-5                  # tests/test_gpu_scene.py: BOUND
FOCAL_BREAK = 20.0
MAX_FLAGGED = 0.10            # the cap: a scene with more flagged pixels tests nothing

# name: (shapes, keyword arguments of make_scene)
SCENES = {
    "3x(2x3)": ([(2, 3)] * 3, dict(seed=2, floater=0.5, focal_scale=2.0)),
    "5x(37x41)": ([(37, 41)] * 5, dict(seed=1)),
    "4x(36x44)": ([(36, 44)] * 4, dict(seed=2)),
    "mixed": ([(32, 48), (24, 40), (32, 48), (24, 40)], dict(seed=3)),
}


def make_scene(shapes, seed=0, floater=0.15, focal_scale=1.25, shared_focal=False):
    """dict(shapes, depth [list of (h,w) float32], c2w [N,4,4] float32, f [N] float32, pp [N,2] float32, K [N,3,3] float32,
    conf [list of (h,w) float32], quat [N,4] (x, y, z, w))."""
    rng = np.random.default_rng(seed)
    N = len(shapes)
    mid = (N - 1) / 2
    depth, conf, c2w, quat = [], [], np.zeros((N, 4, 4)), np.zeros((N, 4))
    f = np.asarray([focal_scale * max(h, w) * (1.0 if shared_focal else 1 + 0.04 * (n - mid)) for n, (h, w) in enumerate(shapes)])
    pp = np.asarray([(w / 2 + 0.7 * np.sin(1.0 + n), h / 2 + 0.6 * np.cos(2.0 + n)) for n, (h, w) in enumerate(shapes)])
    for n, (h, w) in enumerate(shapes):
        a = 0.15 * (n - mid)
        c2w[n] = np.eye(4)
        c2w[n, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[n, :3, 3] = [0.4 * (n - mid), 0.02 * n, 0.0]
        quat[n] = [0, np.sin(a / 2), 0, np.cos(a / 2)]
        xs = np.arange(w)[None, :] * 16.0 / w          # the fixture's 16-pixel-wide wave, whatever the width
        d = 3 + 0.5 * np.sin(xs / 3.0 + n) + np.zeros((h, 1)) + (rng.random((h, w)) < floater) * (-1.5)
        depth.append(d.astype(np.float32))
        conf.append((1 + 5 * rng.random((h, w))).astype(np.float32))
    f32 = lambda a: np.asarray(a, np.float32)
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = f32(f)
    K[:, :2, 2] = f32(pp)
    K[:, 2, 2] = 1
    return dict(shapes=list(shapes), depth=depth, conf=conf, c2w=f32(c2w), f=f32(f), pp=f32(pp), K=K, quat=quat)


def stack(maps, shapes, P=None, fill=0.0):
    """per-image (h,w) maps -> [N,P], `fill` at the padding"""
    P = P or max(h * w for h, w in shapes)
    out = np.full((len(maps), P), fill, np.asarray(maps[0]).dtype)
    for n, (m, (h, w)) in enumerate(zip(maps, shapes)):
        out[n, :h * w] = np.asarray(m).reshape(-1)
    return out


def unstack(rows, shapes):
    return [np.asarray(r)[:h * w].reshape(h, w) for r, (h, w) in zip(rows, shapes)]


def engine_params(sc, mono=None, shifts=None):
    """set_params arguments of the scene.  mono [N,P] (with shifts [N]): the mono form, depth = log((d - shift) / mono)."""
    shapes = sc["shapes"]
    d = stack(sc["depth"], shapes, fill=1.0).astype(np.float64)
    t = sc["c2w"][:, :3, 3].astype(np.float64)
    par = dict(im_poses=np.concatenate([sc["quat"], np.sign(t) * np.log1p(np.abs(t))], 1).astype(np.float32),
               im_focals=(FOCAL_BREAK * np.log(sc["f"].astype(np.float64))).astype(np.float32),
               im_pp=((sc["pp"].astype(np.float64) - np.asarray([(w / 2, h / 2) for h, w in shapes])) / 10).astype(np.float32))
    if mono is None:
        par["depth"] = np.log(d).astype(np.float32)
    else:
        shifts = np.asarray(shifts, np.float64)
        par["depth"] = np.log((d - shifts[:, None]) / np.asarray(mono, np.float64)).astype(np.float32)
        par["shifts"] = shifts.astype(np.float32)
    return par


def world_points(depth, c2w, f, pp, shapes):
    """float64 world points, one (h*w, 3) array per image"""
    out = []
    with np.errstate(all="ignore"):
        for n, (h, w) in enumerate(shapes):
            p = np.arange(h * w)
            x, y, d = (p % w).astype(np.float64), (p // w).astype(np.float64), np.asarray(depth[n], np.float64).reshape(-1)
            rel = np.stack([d * (x - pp[n, 0]) / f[n], d * (y - pp[n, 1]) / f[n], d], 1)
            out.append(rel @ np.asarray(c2w[n], np.float64)[:3, :3].T + np.asarray(c2w[n], np.float64)[:3, 3])
    return out


def oracle(depth, c2w, f, pp, conf, shapes, tol=0.001, bad_conf=0.0, pts=None, sequential=True):
    """(out, flagged, info): out / flagged are lists of (h,w) float32 / bool maps.  depth, conf: lists of (h,w) maps; c2w [N,>=3,4];
    f [N]; pp [N,2]; pts: world points per image instead of the un-projection of `depth`.  sequential=False: every image reads the
    ORIGINAL confidences of all others (what a single launch over all images would compute)."""
    N = len(shapes)
    f, pp, c2w = np.asarray(f, np.float64).reshape(-1), np.asarray(pp, np.float64), np.asarray(c2w, np.float64)
    depth = [np.asarray(d, np.float64) for d in depth]
    orig = [np.asarray(c, np.float32).copy() for c in conf]
    pts = world_points(depth, c2w, f, pp, shapes) if pts is None else [np.asarray(p, np.float64).reshape(-1, 3) for p in pts]
    bad = np.float32(bad_conf)
    keep = 1.0 - float(tol)
    finite_max = max(float(np.abs(p[np.isfinite(p).all(1)]).max()) for p in pts)
    band_z = BOUND * finite_max
    with np.errstate(all="ignore"):
        cam = [[(pts[i] - c2w[j, :3, 3]) @ c2w[j, :3, :3] if i != j else None for j in range(N)] for i in range(N)]
        z_min = min(float(c[:, 2][np.isfinite(c[:, 2]) & (c[:, 2] > band_z)].min()) for row in cam for c in row if c is not None)
        eps_px, eps_rel = 2 * float(f.max()) * BOUND * finite_max / z_min, 10 * BOUND
        out = [c.copy() for c in orig]
        flagged = [np.zeros(s, bool) for s in shapes]
        for i, (h, w) in enumerate(shapes):
            ci = orig[i].reshape(-1).astype(np.float64)
            cand = (ci > float(bad)) & np.isfinite(pts[i]).all(1)                     # NaN confidences: False
            fires = np.zeros(h * w, bool)
            sure = np.zeros(h * w, bool)
            may = np.zeros(h * w, bool)
            for j, (hj, wj) in enumerate(shapes):
                if j == i:
                    continue
                cx, cy, z = cam[i][j].T
                uf, vf = f[j] * cx / z + pp[j, 0], f[j] * cy / z + pp[j, 1]
                fin = np.isfinite(uf) & np.isfinite(vf) & np.isfinite(z)
                u, v = np.rint(np.where(fin, uf, -1.0)), np.rint(np.where(fin, vf, -1.0))     # np.rint: half to even, as torch.round
                vis = fin & (z > 0) & (u >= 0) & (u < wj) & (v >= 0) & (v < hj)
                near_half = lambda t: np.abs(t - np.floor(t) - 0.5) <= eps_px
                reach = (uf > -1) & (uf < wj) & (vf > -1) & (vf < hj)                         # a rounding choice that can matter
                unsure = fin & ((np.abs(z) <= band_z) | ((z > 0) & reach & (near_half(uf) | near_half(vf))))
                q = np.where(vis, v * wj + u, 0).astype(np.int64)
                src = out[j] if (sequential and j < i) else orig[j]
                cj, cj_hi = src.reshape(-1).astype(np.float64)[q], orig[j].reshape(-1).astype(np.float64)[q]
                dj = keep * depth[j].reshape(-1)[q]
                tgt_flag = flagged[j].reshape(-1)[q] if (sequential and j < i) else np.zeros(h * w, bool)
                fires |= cand & vis & (z < dj) & (ci < cj)
                lo, hi = lambda t: t - eps_rel * np.abs(t), lambda t: t + eps_rel * np.abs(t)
                ok = cand & vis & ~unsure
                sure |= ok & ~tgt_flag & (z < lo(dj)) & (ci < lo(cj))
                may |= cand & unsure
                may |= ok & ((z < hi(dj)) | ~np.isfinite(dj)) & (ci < hi(np.where(tgt_flag, cj_hi, cj)))
            o = out[i].reshape(-1)
            o[fires] = bad
            flagged[i] = (may & ~sure).reshape(h, w)
        changed = sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(out, orig))
    total = sum(h * w for h, w in shapes)
    info = dict(eps_px=eps_px, eps_rel=eps_rel, z_min=z_min, flagged=sum(int(m.sum()) for m in flagged) / total, changed=changed / total,
                n_changed=changed, pixels=total)
    return out, flagged, info


def check_agreement(got, conf, out, flagged, bad_conf=0.0):
    """Asserts the agreement rule for per-image maps `got` against the oracle's (out, flagged) and the input `conf`.  Returns the
    number of flagged pixels on which `got` differs from the oracle."""
    bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
    differ = 0
    for n, (g, c, o, m) in enumerate(zip(got, conf, out, flagged)):
        g, c, o = (np.asarray(a, np.float32).reshape(m.shape) for a in (g, c, o))
        wrong = (bits(g) != bits(o)) & ~m
        assert not wrong.any(), (n, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
        with np.errstate(invalid="ignore"):
            clipped = np.where(c > np.float32(bad_conf), np.float32(bad_conf), c)           # min(original, bad_conf); NaN stays
        either = (bits(g) == bits(c)) | (bits(g) == bits(clipped))
        assert either[m].all(), (n, "a flagged pixel holds neither the original nor the clipped value")
        differ += int(((bits(g) != bits(o)) & m).sum())
    return differ


def assert_cap(info):
    """The condition under which a scene is a test at all."""
    assert info["flagged"] <= MAX_FLAGGED, info
    assert info["n_changed"] >= 1, info
