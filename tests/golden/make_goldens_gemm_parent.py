"""Writes gemm_parent.json: what the three matrix-kernel families (csrc/gemm.hip exact fp32, gemm_bf3.hip three-plane bf16, gemm_fh2.hip
two-plane fp16) compute op by op, as the library selected by A3R_LIB (default: the tree's own) computes it on the GPU.  The committed
file pins the results of the commit BEFORE the kernels' tile scaffold, conv geometry, epilogue column preamble, launch helper and
entry checks were shared (csrc/gemm_tile.h, csrc/gemm_common.h):

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_gemm_parent.py [--out FILE]

A case is one (family, forced tile, group of paths); its record maps every path of the group to the SHA-256 of the raw bytes of y, of
any auxiliary output and of the out_absmax word (fh2).  Inputs are seeded numpy.  These are the paths the TINY model of
test_gpu_model_parent.py does not force: every tile (A3R_GEMM_TILE / A3R_BF3_TILE / A3R_FH2_TILE), full (256x256) and ragged
(300x200) tiles, 1-5 k-stages (K = 32..160: the single-step exit, the even and odd tails of the two-step fh2 loop, fewer stages than the
ring), every epilogue and output form, grouped launches, the arithmetic modes, and per conv shape the interior and all four borders
(16x16), stride 2 with one stage per tap (9x7, Cin 32), three stages per tap (Cin 96).

  lin/<family>/<tile>/shapes    M x N in {256x256, 300x200} x K in {32, 64, 96, 128, 160}, bias
  lin/<family>/<tile>/epi       M in {256, 300}, N = 256, K = 64: NONE, GELU, RELU, RESID, RESID2, RESID with relu_acc / relu_out, ROPE with
                                rope_cols 64 / 128 (20 tokens per image, grid_w 5), PIXSHUF (fp32, bf3), HEAD (fh2 tiles 0 and 2, N = 128)
  lin/<family>/<tile>/forms     bf3: out_bf3 plain and row-pair, an x_pair input, aux_bf3 with and without aux_relu; fh2: out_fh2, aux_fh2
                                with and without aux_relu at x_scale 2^3, out_scale 2^-2, and aux_bf3
  lin/<family>/<tile>/grouped   2 and 4 groups of 300x200x64
  lin/bf3/<tile>/products       a3r_bf3_set_products 6 / 3 / 1;  lin/fh2/<tile>/passes: a3r_fh2_set_passes 3 / 1 (restored afterwards)
  conv/<family>/<tile>          (B,H,W,Cin,Cout,stride) in {(1,16,16,64,64,1), (2,9,7,32,128,2), (1,8,8,96,64,1)} x NONE, RELU, RESID2 + aux
  direct_epi                    A3R_BF3_DIRECT_EPI=1: read once per process, so it runs in a fresh child process (this file with
                                `--one NAME OUT`) under the child's own time limit

tests/test_gpu_gemm_parent.py imports CASES and measure_case() from here, so the test and the golden cannot drift apart."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CHILD_TIMEOUT = 300      # seconds: one process start, one library load, a few dozen small GEMMs
CHILD_SWITCHES = ("A3R_BF3_DIRECT_EPI",)      # read once per process
TILE_ENV = {"f32": "A3R_GEMM_TILE", "bf3": "A3R_BF3_TILE", "fh2": "A3R_FH2_TILE"}
TILES = {"f32": ("128x128", "128x64", "64x64"), "bf3": ("0", "1", "2", "3"), "fh2": ("0", "1", "2", "3")}
CONV_TILES = {"f32": TILES["f32"], "bf3": ("0", "1", "2"), "fh2": ("0", "1", "2")}      # tile 3 of bf3 / fh2 is linear-only
CONV_SHAPES = ((1, 16, 16, 64, 64, 1), (2, 9, 7, 32, 128, 2), (1, 8, 8, 96, 64, 1))
X_SCALE, OUT_SCALE = 8.0, 0.25

CASES = {}
for _f in TILES:
    for _t in TILES[_f]:
        for _g in ("shapes", "epi", "forms", "grouped") + (("products",) if _f == "bf3" else ("passes",) if _f == "fh2" else ()):
            if not (_f == "f32" and _g == "forms"):
                CASES[f"lin/{_f}/{_t}/{_g}"] = dict(family=_f, tile=_t, group=_g, child={})
    for _t in CONV_TILES[_f]:
        CASES[f"conv/{_f}/{_t}"] = dict(family=_f, tile=_t, group="conv", child={})
CASES["direct_epi"] = dict(family="bf3", tile=None, group="direct_epi", child={"A3R_BF3_DIRECT_EPI": "1"})       # the child process last


def _rand(tag, shape, scale=1.0):
    r = np.random.default_rng(zlib.crc32(tag.encode()))
    return (scale * r.standard_normal(shape)).astype(np.float32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.data if hasattr(t, "data_ptr") and not hasattr(t, "cpu") else t          # ops.Bf3 / ops.Fh2 -> their storage
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


class _Env:
    def __init__(self, var, val):
        self.var, self.val = var, val

    def __enter__(self):
        self.saved = os.environ.get(self.var)
        os.environ.pop(self.var, None)
        if self.val is not None:
            os.environ[self.var] = self.val

    def __exit__(self, *exc):
        os.environ.pop(self.var, None)
        if self.saved is not None:
            os.environ[self.var] = self.saved


def _rope_tables():
    p, d = np.arange(256, dtype=np.float64)[:, None], np.arange(16, dtype=np.float64)[None, :]
    ang = p / 100.0 ** (d / 16.0)
    return _dev(np.cos(ang).astype(np.float32)), _dev(np.sin(ang).astype(np.float32))


def _operands(fam, tag, M, N, K):
    """(x, w) of one problem in the family's operand form, and the bias"""
    from align3r_amd import ops
    x, w = _dev(_rand(tag + "x", (M, K))), _dev(_rand(tag + "w", (N, K), K ** -0.5))
    bias = _dev(_rand(tag + "b", (N,)))
    if fam == "bf3":
        return ops.split_bf3(x), ops.split_bf3_w(w), bias
    if fam == "fh2":
        return ops.split_fh2(x, X_SCALE), ops.split_fh2_w(w), bias
    return x, w, bias


def _linear(fam, tag, M, N, K, epi=0, **kw):
    """one linear launch -> the digest of everything it wrote"""
    import torch
    from align3r_amd import ops
    x, w, bias = _operands(fam, tag, M, N, K)
    fn = {"f32": ops.linear, "bf3": ops.linear_bf3, "fh2": ops.linear_fh2}[fam]
    extra = []
    if fam == "fh2":
        kw["out_absmax"] = ops.absmax_word("cuda")
        extra.append(kw["out_absmax"])
        if kw.get("out_fh2") or kw.get("aux_fh2") is not None:
            kw["out_scale"] = OUT_SCALE
    for k in ("aux_bf3", "aux_fh2"):
        if kw.get(k) is not None:
            extra.append(kw[k])
    if kw.get("head") is not None:
        extra.append(kw["head"][2])
    if "out" not in kw and not kw.get("out_bf3") and not kw.get("out_fh2"):
        kw["out"] = torch.zeros((M, N), device="cuda", dtype=torch.float32)
    y = fn(x, w, bias, epi=epi, **kw)
    return _sha(y, *extra), y


def _epi_paths(fam, tile, tag):
    import torch
    from align3r_amd import _lib as L
    from align3r_amd import ops
    cos, sin = _rope_tables()
    rec = {}
    for M in (256, 300):
        N, K = 256, 64
        t = f"{tag}{M}"
        r1, r2 = _dev(_rand(t + "r1", (M, N))), _dev(_rand(t + "r2", (M, N)))
        for name, epi, kw in (("none", L.EPI_NONE, {}), ("gelu", L.EPI_GELU, {}), ("relu", L.EPI_RELU, {}), ("resid", L.EPI_RESID, dict(resid=r1)),
                              ("resid2", L.EPI_RESID2, dict(resid=r1, resid2=r2)), ("resid_relu_acc", L.EPI_RESID, dict(resid=r1, relu_acc=True)),
                              ("resid_relu_out", L.EPI_RESID, dict(resid=r1, relu_out=True)),
                              ("rope64", L.EPI_ROPE, dict(rope=(64, 20, 5, cos, sin))), ("rope128", L.EPI_ROPE, dict(rope=(128, 20, 5, cos, sin)))):
            rec[f"{name}/{M}"] = _linear(fam, t, M, N, K, epi, **kw)[0]
        if fam != "fh2":
            hw, side = (64, 8) if M == 256 else (100, 10)
            out = torch.zeros((M // hw, 2 * side, 2 * side, 64), device="cuda", dtype=torch.float32)
            rec[f"pixshuf/{M}"] = _linear(fam, t, M, N, K, L.EPI_PIXSHUF, out=out, pixshuf=(2, side, side, 64))[0]
        elif tile in ("0", "2"):
            head = (_dev(_rand(t + "hw", (4, 128), 0.05)), _dev(_rand(t + "hb", (4,), 0.1)), torch.zeros(M, device="cuda", dtype=torch.float32))
            rec[f"head/{M}"] = _linear(fam, t + "h", M, 128, K, L.EPI_HEAD, head=head)[0]
    return rec


def _form_paths(fam, tag):
    import torch
    from align3r_amd import _lib as L
    from align3r_amd import ops
    cos, sin = _rope_tables()
    rec = {}
    for M in (256, 300):
        N, K = 256, 64
        t = f"{tag}{M}"
        r1 = _dev(_rand(t + "r1", (M, N)))
        aux3 = lambda: ops.Bf3(torch.zeros(M * N * 6, device="cuda", dtype=torch.uint8), M, N)
        if fam == "bf3":
            for name, epi, kw in (("none", L.EPI_NONE, {}), ("gelu", L.EPI_GELU, {}), ("rope64", L.EPI_ROPE, dict(rope=(64, 20, 5, cos, sin)))):
                rec[f"out_bf3/{name}/{M}"] = _linear(fam, t, M, N, K, epi, out_bf3=True, **kw)[0]
                rec[f"out_pair/{name}/{M}"], y3p = _linear(fam, t, M, N, K, epi, out_bf3=True, out_pair=True, **kw)
            w2 = ops.split_bf3_w(_dev(_rand(t + "w2", (200, N), N ** -0.5)))              # the row-pair output as the next GEMM's x_pair input
            rec[f"x_pair/{M}"] = _sha(ops.linear_bf3(y3p, w2, None))
            rec[f"x_pair/gelu_out_bf3/{M}"] = _sha(ops.linear_bf3(y3p, w2, None, epi=L.EPI_GELU, out_bf3=True))
        else:
            for name, epi, kw in (("none", L.EPI_NONE, {}), ("gelu", L.EPI_GELU, {}), ("relu", L.EPI_RELU, {}),
                                  ("rope64", L.EPI_ROPE, dict(rope=(64, 20, 5, cos, sin))), ("rope128", L.EPI_ROPE, dict(rope=(128, 20, 5, cos, sin)))):
                rec[f"out_fh2/{name}/{M}"] = _linear(fam, t, M, N, K, epi, out_fh2=True, **kw)[0]
            for name, epi, kw in (("none", L.EPI_NONE, {}), ("resid", L.EPI_RESID, dict(resid=r1)), ("resid_relu", L.EPI_RESID, dict(resid=r1, aux_relu=True))):
                aux2 = ops.Fh2(torch.zeros(M * N * 4, device="cuda", dtype=torch.uint8), M, N, OUT_SCALE)
                rec[f"aux_fh2/{name}/{M}"] = _linear(fam, t, M, N, K, epi, aux_fh2=aux2, **kw)[0]
        for name, epi, kw in (("none", L.EPI_NONE, {}), ("resid", L.EPI_RESID, dict(resid=r1)), ("resid_relu", L.EPI_RESID, dict(resid=r1, aux_relu=True)),
                              ("gelu_relu", L.EPI_GELU, dict(aux_relu=True))):
            rec[f"aux_bf3/{name}/{M}"] = _linear(fam, t, M, N, K, epi, aux_bf3=aux3(), **kw)[0]
    return rec


def _grouped_paths(fam, tag):
    from align3r_amd import _lib as L
    from align3r_amd import ops
    M, N, K = 300, 200, 64
    rec = {}
    for G in (2, 4):
        prob = [_operands(fam, f"{tag}{G}.{i}", M, N, K) for i in range(G)]
        resid = [_dev(_rand(f"{tag}{G}.{i}r", (M, N))) for i in range(G)]
        xs, ws, bs = [p[0] for p in prob], [p[1] for p in prob], [p[2] for p in prob]
        fn = {"f32": ops.linear_grouped, "bf3": ops.linear_bf3_grouped, "fh2": ops.linear_fh2_grouped}[fam]
        rec[f"none/{G}"] = _sha(*fn(xs, ws, bs))
        rec[f"resid/{G}"] = _sha(*fn(xs, ws, bs, epi=L.EPI_RESID, resids=resid))
    return rec


def _conv_paths(fam, tag):
    import torch
    from align3r_amd import _lib as L
    from align3r_amd import ops
    rec = {}
    for B, H, W, Cin, Cout, stride in CONV_SHAPES:
        t = f"{tag}{H}x{W}"
        x = _dev(_rand(t + "x", (B, H, W, Cin)))
        wp = _dev(_rand(t + "w", (Cout, 3, 3, Cin), (9 * Cin) ** -0.5))
        bias = _dev(_rand(t + "b", (Cout,)))
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = B * Ho * Wo
        r1, r2 = _dev(_rand(t + "r1", (M, Cout))), _dev(_rand(t + "r2", (M, Cout)))
        for name, epi, kw in (("none", L.EPI_NONE, {}), ("relu", L.EPI_RELU, {}), ("resid2_aux", L.EPI_RESID2, dict(resid=r1, resid2=r2))):
            extra = []
            if fam == "f32":
                y = ops.conv3x3(x, wp, bias, stride, epi, **kw)
            elif fam == "bf3":
                if epi == L.EPI_RESID2:
                    kw = dict(kw, aux_bf3=ops.Bf3(torch.zeros(M * Cout * 6, device="cuda", dtype=torch.uint8), M, Cout), aux_relu=True)
                    extra.append(kw["aux_bf3"])
                y = ops.conv3x3_bf3(ops.split_bf3(x), ops.split_bf3_w(wp.reshape(Cout, 9 * Cin)), (B, H, W, Cin), bias, stride, epi, **kw)
            else:
                word = ops.absmax_word("cuda")
                extra.append(word)
                if epi == L.EPI_RESID2:
                    kw = dict(kw, aux_fh2=ops.Fh2(torch.zeros(M * Cout * 4, device="cuda", dtype=torch.uint8), M, Cout, OUT_SCALE), aux_relu=True,
                              out_scale=OUT_SCALE)
                    extra.append(kw["aux_fh2"])
                y = ops.conv3x3_fh2(ops.split_fh2(x, X_SCALE), ops.split_fh2_w(wp.reshape(Cout, 9 * Cin)), (B, H, W, Cin), bias, stride, epi,
                                    out_absmax=word, **kw)
            rec[f"{B}x{H}x{W}x{Cin}x{Cout}s{stride}/{name}"] = _sha(y, *extra)
        if fam == "f32":
            rec[f"{B}x{H}x{W}x{Cin}x{Cout}s{stride}/relu_a"] = _sha(ops.conv3x3(x, wp, bias, stride, relu_a=True))
    return rec


def _measure_here(name):
    from align3r_amd import ops
    case = CASES[name]
    for k in CHILD_SWITCHES:
        assert os.environ.get(k) == case["child"].get(k), (name, k, os.environ.get(k))
    fam, tile, group = case["family"], case["tile"], case["group"]
    if group == "direct_epi":          # the accumulator-layout epilogue of the bf3 kernels on every tile that has the LDS form
        rec = {}
        for t in ("0", "1", "2"):
            with _Env(TILE_ENV["bf3"], t):
                for k, v in list(_epi_paths("bf3", t, name).items()) + list(_form_paths("bf3", name).items()):
                    rec[f"{t}/{k}"] = v
        return rec
    with _Env(TILE_ENV[fam], tile):
        if group == "shapes":
            return {f"{M}x{N}x{K}": _linear(fam, f"{name}{M}.{K}", M, N, K)[0] for M, N in ((256, 256), (300, 200)) for K in (32, 64, 96, 128, 160)}
        if group == "epi":
            return _epi_paths(fam, tile, name)
        if group == "forms":
            return _form_paths(fam, name)
        if group == "grouped":
            return _grouped_paths(fam, name)
        if group == "conv":
            return _conv_paths(fam, name)
        setter, modes = (ops.bf3_set_products, (6, 3, 1)) if group == "products" else (ops.fh2_set_passes, (3, 1))
        rec = {}
        prev = setter(modes[0])
        try:
            for m in modes:
                setter(m)
                for M, N in ((256, 256), (300, 200)):
                    for K in (32, 96):
                        rec[f"{m}/{M}x{N}x{K}"] = _linear(fam, f"{name}{M}.{K}", M, N, K)[0]
        finally:
            setter(prev)
        return rec


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
    dst = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(HERE, "gemm_parent.json")
    records = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:       # the child process is the last one
            records[name] = measure_case(name, tmp)
            print(name, "ok", len(records[name]), flush=True)
    with open(dst, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(records)} cases to {dst}")
