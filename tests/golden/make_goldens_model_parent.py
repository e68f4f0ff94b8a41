"""Writes model_parent.json: what the pair network's launch plan computes, as the library selected by A3R_LIB (default: the tree's
own) computes it on the GPU.  The committed file pins the results of the commit BEFORE the plan was split into stages and the
fp32 DPT head was put onto the operand-form path (csrc/model.hip):

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_model_parent.py [--out FILE]

Per case, on a fresh PairEngine (TINY, synthetic_state_dict(TINY, 0)) after reset_ranges(): the SHA-256 of the raw bytes of every
output (pts3d_1, conf_1, pts3d_2, conf_2; feat for encode), of site_scales(phase) and of site_stats(), and the tuples last_dedup()
and last_dedup_sides().  The order of the plan's allocations and fh2 sites is observable through exactly these,
so equal digests mean an unchanged plan.  The cases:

  fwd/<mode>/1x48x80, 2x64x96   every arithmetic mode; 48x80 has N = 15 tokens per frame (odd rows: no bf3 pair mode, cropped maps)
  dup*/<mode>/<size>            B = 5 from three frames, I1, I2 = [0,0,1,2,1], [1,2,0,0,2]: images, depth priors and (fh2 maps) both
                                heads merge; dup_pd: the same with all ten depth priors distinct; dup_img: all ten images distinct
                                and the priors repeated
  encdec/<mode>                 encode of 3 frames at 64x96, then decode of the I1 / I2 batches of those features
  fold0, tap3, dedup0, dedup2   A3R_DEDUP_HEAD_FOLD=0, set_tap_level(3) (with the taps level, pc0, hook_a, hook_b, dec_last),
                                set_dedup(0) and set_dedup(2)
  ref_order, plain_act          A3R_DPT_REF_ORDER=1 and A3R_BF3_PLAIN_ACT=1: read once per process, so each runs in a fresh child
                                process (this file with `--one NAME OUT`) under the child's own time limit

tests/test_gpu_model_parent.py imports CASES and measure_case() from here, so the test and the golden cannot drift apart."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CHILD_TIMEOUT = 300      # seconds: one process start, one library load, one TINY forward of two pairs
I1, I2 = [0, 0, 1, 2, 1], [1, 2, 0, 0, 2]         # B = 5 from 3 frames, sides swapped
# (A3R_GEMM, A3R_CONV), None = unset: both are read when the handle is made
MODES = {"unset": (None, None), "f16": ("f16", None), "bf3": ("bf3", None), "f32": ("f32", None), "conv_bf3": (None, "bf3")}
CHILD_SWITCHES = ("A3R_DPT_REF_ORDER", "A3R_BF3_PLAIN_ACT")      # read once per process


def _case(mode, kind, H=64, W=96, env=None, child=None, **kw):
    return dict(mode=mode, kind=kind, H=H, W=W, env=env or {}, child=child or {}, **kw)


CASES = {}
for _m in MODES:
    CASES[f"fwd/{_m}/1x48x80"] = _case(_m, "fwd", 48, 80, B=1)
    CASES[f"fwd/{_m}/2x64x96"] = _case(_m, "fwd", B=2)
for _m in ("unset", "f32", "bf3"):
    for _H, _W in ((64, 96), (48, 80)):
        for _k in ("dup", "dup_pd", "dup_img"):
            CASES[f"{_k}/{_m}/{_H}x{_W}"] = _case(_m, _k, _H, _W)
for _m in ("unset", "f32"):
    CASES[f"encdec/{_m}"] = _case(_m, "encdec")
CASES["fold0"] = _case("unset", "dup", env={"A3R_DEDUP_HEAD_FOLD": "0"})
CASES["tap3"] = _case("unset", "fwd", B=2, tap=3)
CASES["dedup0"] = _case("unset", "dup", dedup=0)
CASES["dedup2"] = _case("unset", "dup", dedup=2)
CASES["ref_order"] = _case("unset", "fwd", B=2, child={"A3R_DPT_REF_ORDER": "1"})          # the child processes last
CASES["plain_act"] = _case("bf3", "fwd", B=2, child={"A3R_BF3_PLAIN_ACT": "1"})


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _frames(n, H, W, seed=3):
    """n synthetic frames (image [3,H,W], pred_depth [H,W,3]) on the device: the frames of conftest.make_view_arrays"""
    import torch
    from align3r_amd.weights import hash_uniform
    img = [torch.from_numpy((2.0 * hash_uniform(f"img{i}", 3 * H * W, seed)).astype(np.float32).reshape(3, H, W)).cuda() for i in range(n)]
    pd = [torch.from_numpy((hash_uniform(f"pred_depth{i}", H * W * 3, seed) + 0.5).astype(np.float32).reshape(H, W, 3)).cuda() for i in range(n)]
    return img, pd


def _batch(items, idx):
    import torch
    return torch.stack([items[i] for i in idx]).contiguous()


_SD = None


def _engine(case):
    """a fresh engine made under the case's environment"""
    global _SD
    from align3r_amd.engine import PairEngine
    from align3r_amd.weights import TINY, synthetic_state_dict
    if _SD is None:
        _SD = synthetic_state_dict(TINY, 0)
    gemm, conv = MODES[case["mode"]]
    want = dict({"A3R_GEMM": gemm, "A3R_CONV": conv, "A3R_DEDUP": None, "A3R_DEDUP_HEAD": None, "A3R_DEDUP_HEAD_FOLD": None}, **case["env"])
    saved = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        e = PairEngine(TINY, _SD)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    e.reset_ranges()
    return e


def _state(e, phase, out):
    rec = {k: _sha(v.cpu().numpy()) for k, v in out.items()}
    rec["site_scales"] = _sha(e.site_scales(phase))
    rec["site_stats"] = _sha(e.site_stats())
    rec["n_sites"] = int(e.site_scales(phase).size)
    rec["last_dedup"] = list(e.last_dedup())
    rec["last_dedup_sides"] = list(e.last_dedup_sides())
    return rec


def _measure_here(name):
    from align3r_amd.weights import TINY
    case = CASES[name]
    for k in CHILD_SWITCHES:
        assert os.environ.get(k) == case["child"].get(k), (name, k, os.environ.get(k))
    H, W, kind = case["H"], case["W"], case["kind"]
    e = _engine(case)
    if "dedup" in case:
        e.set_dedup(case["dedup"])
    if "tap" in case:
        e.set_tap_level(case["tap"])
    if kind == "fwd":
        B = case["B"]
        img, pd = _frames(2 * B, H, W)
        i1, i2 = list(range(B)), list(range(B, 2 * B))
        rec = _state(e, 0, e.forward(_batch(img, i1), _batch(img, i2), _batch(pd, i1), _batch(pd, i2)))
        if "tap" in case:
            for tap, cols in (("level", TINY.dec_embed_dim), ("pc0", TINY.dec_embed_dim), ("hook_a", TINY.dec_embed_dim),
                              ("hook_b", TINY.dec_embed_dim), ("dec_last", TINY.dec_embed_dim)):
                rec["tap_" + tap] = _sha(e.tap(tap, cols).cpu().numpy())
        return rec
    img, pd = _frames(10, H, W)
    d1, d2 = list(range(5)), list(range(5, 10))
    if kind == "encdec":
        feat = e.encode(_batch(img, [0, 1, 2]))
        rec = {"encode": _state(e, 1, {"feat": feat})}
        rec["decode"] = _state(e, 2, e.decode(_batch(feat, I1), _batch(feat, I2), _batch(pd, I1), _batch(pd, I2), H, W))
        return rec
    im1, im2 = (d1, d2) if kind == "dup_img" else (I1, I2)
    p1, p2 = (d1, d2) if kind == "dup_pd" else (I1, I2)
    return _state(e, 0, e.forward(_batch(img, im1), _batch(img, im2), _batch(pd, p1), _batch(pd, p2)))


def measure_case(name, scratch_dir):
    """the record of one case from the loaded library; a case that needs a once-per-process switch runs in a fresh child process that
    leaves its record in scratch_dir"""
    child = CASES[name]["child"]
    if all(os.environ.get(k) == child.get(k) for k in CHILD_SWITCHES):
        return _measure_here(name)
    out = os.path.join(scratch_dir, name.replace("/", "_") + ".json")
    env = {k: v for k, v in os.environ.items() if k not in CHILD_SWITCHES}
    env.update(child)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the child process of case {name} ended with status {r.returncode}:\n{r.stdout}")
    with open(out) as f:
        return json.load(f)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        with open(sys.argv[3], "w") as f:
            json.dump(_measure_here(sys.argv[2]), f)
        sys.exit(0)
    import tempfile
    dst = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(HERE, "model_parent.json")
    records = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:       # the child processes are the last ones
            records[name] = measure_case(name, tmp)
            print(name, "ok", flush=True)
    with open(dst, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(records)} cases to {dst}")
