"""Writes producers_parent.json: what the memory-bound producers of csrc/elementwise.hip (LayerNorm in its three output forms, the
bilinear 2x in its forms, the residual combine, the gather-add with two sources) and the Umeyama moments kernel compute, as the
library selected by A3R_LIB (default: the tree's own) computes it on the GPU.  The committed file pins the results of the commit
BEFORE the kernels of that file were put on shared helpers and the moments kernel moved to csrc/init.hip:

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_producers_parent.py [--out FILE]

A case is one (entry, shape); its record maps every call of the case to the SHA-256 of the raw bytes of all of the call's outputs,
the statistics word included.  Outputs are pre-filled with NaN (fp32) or 0xFF bytes (packed forms) and carry a guard tail, so the
bytes a call must leave alone are part of the digest.  Every output element is written once from per-element arithmetic and the
statistics word is an integer maximum, so a record is the same in every run.  Inputs: numpy.random.default_rng(seed) on the host.

  ln/<M>x<D>                  a3r_layernorm: the register kernels (D = 1024, 768, 256) and the generic one
  ln_bf3/<M>x<D>              a3r_layernorm_bf3 plain and, where D % 32 == 0, row-pair (M odd: the partner of the last row stays sentinel)
  ln_fh2/<M>x<D>[u]           a3r_layernorm_fh2 with and without the word at scales 1 and 2^-5; u: x 4 bytes off alignment (generic);
                              16391x32: with the word only, the second trip of the persistent loop
  up/<shape>                  a3r_upsample2x and a3r_upsample2x_fh2 (with word) under both forms, a3r_upsample2x_bf3 (one form)
  upc/<i>, upc_src/<i>        a3r_upsample2x_combine_fh2 / _src under both forms; _src mixes stored entries (stride > Hc Wc C) and fresh blocks
  comb/<S>x<U>x<P>x<C>        a3r_combine_resid_fh2 and _src; 5x2x1000x1024: the second trip of the persistent loop
  gadd_src                    a3r_gather_add_rows_src with b and in place
  umeyama/<P>                 a3r_umeyama_moments, B = 2

tests/test_gpu_producers_parent.py imports CASES and measure_case() from here, so the test and the golden cannot drift apart."""
import ctypes as C
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

from test_gpu_up2x_forms import SHAPES as UP_SHAPES        # noqa: E402

EPS = 1e-6
LN_F32 = [(5, 1024), (5, 768), (5, 256), (3, 36), (5, 1280)]
LN_BF3 = [(7, 1024), (7, 768), (7, 256), (5, 40), (6, 32), (5, 1280)]
LN_FH2_D = [32, 480, 512, 544, 1024, 1056, 1536, 1568]
LN_FH2_PERSISTENT = (16391, 32)
# (S, U, H, W, C, crop, map): the cases of test_gpu_up2x_forms.test_combine_forms_are_bitwise_equal
UPC = [(3, 2, 3, 5, 8, (5, 10), [1, 1, 0]), (4, 2, 4, 6, 256, None, [0, 1, 1, 0]), (2, 1, 1, 1, 16, None, [0, 0]),
       (3, 3, 9, 20, 128, (17, 39), [2, 0, 1])]
COMB = [(3, 2, 5, 8), (4, 2, 7, 256), (5, 2, 1000, 1024)]
UMEYAMA_P = (1, 1023, 1025)

CASES = {}
for _M, _D in LN_F32:
    CASES[f"ln/{_M}x{_D}"] = dict(family="ln", M=_M, D=_D)
for _M, _D in LN_BF3:
    CASES[f"ln_bf3/{_M}x{_D}"] = dict(family="ln_bf3", M=_M, D=_D)
for _D in LN_FH2_D:
    CASES[f"ln_fh2/5x{_D}"] = dict(family="ln_fh2", M=5, D=_D)
CASES["ln_fh2/5x256u"] = dict(family="ln_fh2", M=5, D=256, unaligned=True)
CASES["ln_fh2/%dx%d" % LN_FH2_PERSISTENT] = dict(family="ln_fh2", M=LN_FH2_PERSISTENT[0], D=LN_FH2_PERSISTENT[1], word_only=True)
for _i, _s in enumerate(UP_SHAPES):
    CASES[f"up/{_i}"] = dict(family="up", shape=_s, seed=300 + _i)
for _i, _s in enumerate(UPC):
    CASES[f"upc/{_i}"] = dict(family="upc", shape=_s, seed=400 + _i, src=False)
    CASES[f"upc_src/{_i}"] = dict(family="upc", shape=_s, seed=400 + _i, src=True)
for _s in COMB:
    CASES["comb/%dx%dx%dx%d" % _s] = dict(family="comb", shape=_s)
CASES["gadd_src"] = dict(family="gadd_src")
for _P in UMEYAMA_P:
    CASES[f"umeyama/{_P}"] = dict(family="umeyama", P=_P)


def _torch():
    import torch
    return torch


def _lib():
    from align3r_amd import _lib as lib
    return lib


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nan(n):
    """fp32 output of n elements and a guard tail, NaN-filled"""
    return _torch().full((n + 16,), float("nan"), device="cuda")


def _ff(nbytes):
    """packed output of nbytes and a guard tail, 0xFF-filled"""
    return _torch().full((nbytes + 64,), 0xFF, dtype=_torch().uint8, device="cuda")


def _word():
    return _torch().zeros(1, dtype=_torch().int32, device="cuda")


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"<none>")
        else:
            h.update(repr(tuple(t.shape)).encode())
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def _call(name, *args):
    lib = _lib()
    lib.check(getattr(lib.load(), name)(*args, lib.stream_ptr()), name)


def _both_forms(rec, tag, run):
    """rec[tag/form] = run() under form 1 and form 2; the process-wide switch is put back"""
    lib = _lib().load()
    prev = lib.a3r_upsample2x_set_form(2)
    assert prev in (1, 2)
    try:
        for form in (1, 2):
            assert lib.a3r_upsample2x_set_form(form) in (1, 2)
            rec[f"{tag}/form{form}"] = run()
    finally:
        lib.a3r_upsample2x_set_form(prev)


def _f32(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def _ln_inputs(M, D, seed):
    rng = np.random.default_rng(seed)
    x = _f32(rng, M, D, scale=3.0) + _f32(rng, M, 1)
    return _dev(x), _dev(1 + 0.5 * _f32(rng, D)), _dev(_f32(rng, D))


# ------------------------------------------------------------------------------------------------- LayerNorm
def _ln(case):
    M, D = case["M"], case["D"]
    x, w, b = _ln_inputs(M, D, 10000 * M + D)
    y = _nan(M * D)
    _call("a3r_layernorm", _p(x), _p(w), _p(b), _p(y), M, D, EPS)
    return {"y": _sha(y)}


def _ln_bf3(case):
    M, D = case["M"], case["D"]
    x, w, b = _ln_inputs(M, D, 10000 * M + D + 1)
    rec = {}
    for pair in (0, 1):
        if pair and D % 32:
            continue
        y3 = _ff((M + (M & 1) if pair else M) * D * 6)
        _call("a3r_layernorm_bf3", _p(x), _p(w), _p(b), _p(y3), M, D, EPS, pair)
        rec["pair" if pair else "plain"] = _sha(y3)
    return rec


def _ln_fh2(case):
    torch = _torch()
    M, D = case["M"], case["D"]
    x, w, b = _ln_inputs(M, D, 10000 * M + D + 2)
    if case.get("unaligned"):
        big = torch.zeros(M * D + 8, device="cuda")
        xu = big[1:1 + M * D].view(M, D)
        xu.copy_(x)
        assert xu.data_ptr() % 16 == 4
        x = xu
    rec = {}
    for scale in (1.0, 2.0 ** -5):
        for with_word in (True,) if case.get("word_only") else (True, False):
            y2, word = _ff(M * D * 4), _word() if with_word else None
            _call("a3r_layernorm_fh2", _p(x), _p(w), _p(b), _p(y2), M, D, EPS, scale, _p(word))
            rec[f"s={scale:g}/{'word' if with_word else 'none'}"] = _sha(y2, word)
    return rec


# ------------------------------------------------------------------------------------------------- bilinear 2x
def _up(case):
    B, H, W, Cc, crop = case["shape"]
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    x = _dev(_f32(np.random.default_rng(case["seed"]), B, H, W, Cc, scale=3.0))
    n = B * Hc * Wc * Cc
    rec = {}

    def fp32():
        y = _nan(n)
        _call("a3r_upsample2x", _p(x), _p(y), B, H, W, Cc, Hc, Wc)
        return _sha(y)

    def fh2():
        y2, word = _ff(n * 4), _word()
        _call("a3r_upsample2x_fh2", _p(x), _p(y2), B, H, W, Cc, Hc, Wc, 4.0, _p(word))
        return _sha(y2, word)
    _both_forms(rec, "fp32", fp32)
    _both_forms(rec, "fh2", fh2)
    y3 = _ff(n * 6)
    _call("a3r_upsample2x_bf3", _p(x), _p(y3), B, H, W, Cc, Hc, Wc)
    rec["bf3"] = _sha(y3)
    return rec


def _stored(rng, blocks, words, n_ent):
    """the row blocks [n, words] of `blocks` as a storage of n_ent entries `stride` floats apart (stride > words), filled with
    other numbers; returns the storage, the stride and which entry holds block k (entries are dealt in reverse)"""
    stride = words + 64
    store = _f32(rng, n_ent, stride)
    where = [n_ent - 1 - k for k in range(blocks.shape[0])]
    for k, e in enumerate(where):
        store[e, :words] = blocks[k].reshape(-1)
    return store, stride, where


def _signed_sources(idx, where):
    """slot b reads block idx[b]: from the storage for even b (entry >= 0), from the fresh blocks for odd b (~block < 0)"""
    return np.array([where[k] if b % 2 == 0 else ~k for b, k in enumerate(idx)], dtype=np.int32)


def _upc(case):
    S, U, H, W, Cc, crop, idx = case["shape"]
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    rng = np.random.default_rng(case["seed"])
    x, c, r0 = _f32(rng, S, H, W, Cc, scale=3.0), _f32(rng, U, Hc, Wc, Cc, scale=3.0), _f32(rng, U, Hc, Wc, Cc, scale=3.0)
    words = Hc * Wc * Cc
    if case["src"]:
        sc, stride, where = _stored(rng, c, words, U + 1)
        sr, _, _ = _stored(rng, r0, words, U + 1)
        sc, sr, m = _dev(sc), _dev(sr), _dev(_signed_sources(idx, where))
        assert int((m >= 0).sum()) > 0 and (S == 1 or int((m < 0).sum()) > 0)
    else:
        m = _dev(np.array(idx, dtype=np.int32))
    x, c, r0 = _dev(x), _dev(c), _dev(r0)

    def run():
        s, sr2, word = _nan(S * words), _ff(S * words * 4), _word()
        if case["src"]:
            _call("a3r_upsample2x_combine_fh2_src", _p(x), _p(c), _p(r0), _p(sc), _p(sr), stride, _p(m), _p(s), _p(sr2), S, H, W, Cc, Hc, Wc,
                  2.0, _p(word))
        else:
            _call("a3r_upsample2x_combine_fh2", _p(x), _p(c), _p(r0), _p(m), _p(s), _p(sr2), S, H, W, Cc, Hc, Wc, 2.0, _p(word))
        return _sha(s, sr2, word)
    rec = {}
    _both_forms(rec, "combine", run)
    return rec


# ------------------------------------------------------------------------------------------------- residual combine
def _comb(case):
    S, U, P, Cc = case["shape"]
    rng = np.random.default_rng(500 + P)
    c, r0, p2 = _f32(rng, U, P, Cc, scale=3.0), _f32(rng, U, P, Cc, scale=3.0), _f32(rng, S, P, Cc, scale=3.0)
    idx = [b % U for b in range(S)][::-1]
    sc, stride, where = _stored(rng, c, P * Cc, U + 1)
    sr, _, _ = _stored(rng, r0, P * Cc, U + 1)
    m, src = _dev(np.array(idx, dtype=np.int32)), _dev(_signed_sources(idx, where))
    c, r0, p2, sc, sr = _dev(c), _dev(r0), _dev(p2), _dev(sc), _dev(sr)
    rec = {}
    for tag in ("map", "src"):
        s, sr2, word = _nan(S * P * Cc), _ff(S * P * Cc * 4), _word()
        if tag == "src":
            _call("a3r_combine_resid_fh2_src", _p(c), _p(r0), _p(sc), _p(sr), stride, _p(src), _p(p2), _p(s), _p(sr2), S, P, Cc, 0.5, _p(word))
        else:
            _call("a3r_combine_resid_fh2", _p(c), _p(r0), _p(p2), _p(m), _p(s), _p(sr2), S, P, Cc, 0.5, _p(word))
        rec[tag] = _sha(s, sr2, word)
    return rec


# ------------------------------------------------------------------------------------------------- gather-add, two sources
def _gadd_src(case):
    S, N, Cc, F, Ub = 5, 7, 12, 2, 3
    rng = np.random.default_rng(600)
    fresh, b, dst0 = _f32(rng, F, N, Cc), _f32(rng, Ub, N, Cc), _f32(rng, S * N * Cc)
    idx = [1, 0, 0, 1, 1]
    store, stride, where = _stored(rng, fresh, N * Cc, F + 2)
    src, mb = _dev(_signed_sources(idx, where)), _dev(np.array([2, 0, 1, 1, 2], dtype=np.int32))
    store, fresh, b = _dev(store), _dev(fresh), _dev(b)
    rec = {}
    for tag in ("b", "in_place"):
        dst = _nan(S * N * Cc)
        if tag == "in_place":
            dst[:S * N * Cc] = _dev(dst0)
        _call("a3r_gather_add_rows_src", _p(store), stride, _p(fresh), _p(src), _p(b) if tag == "b" else None, _p(mb) if tag == "b" else None,
              _p(dst), S, N, Cc)
        rec[tag] = _sha(dst)
    return rec


# ------------------------------------------------------------------------------------------------- Umeyama moments
def _umeyama(case):
    torch = _torch()
    P, B = case["P"], 2
    rng = np.random.default_rng(700 + P)
    x, y, w = _dev(_f32(rng, B, P, 3)), _dev(_f32(rng, B, P, 3)), _dev(rng.random((B, P)).astype(np.float32))
    xo, wo = _dev(np.arange(B, dtype=np.int64) * 3 * P), _dev(np.arange(B, dtype=np.int64) * P)
    nch = _lib().load().a3r_umeyama_chunks(P)
    part = torch.full((B * nch * 17 + 8,), float("nan"), dtype=torch.float64, device="cuda")
    _call("a3r_umeyama_moments", _p(x), _p(y), _p(w), _p(xo), _p(xo), _p(wo), B, P, _p(part))
    return {"partial": _sha(part)}


_FAMILIES = dict(ln=_ln, ln_bf3=_ln_bf3, ln_fh2=_ln_fh2, up=_up, upc=_upc, comb=_comb, gadd_src=_gadd_src, umeyama=_umeyama)


def measure_case(name):
    """the record of one case from the loaded library"""
    case = CASES[name]
    return _FAMILIES[case["family"]](case)


if __name__ == "__main__":
    import time
    dst = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(HERE, "producers_parent.json")
    records = {}
    for name in CASES:
        t0 = time.time()
        records[name] = measure_case(name)
        print(name, "ok", len(records[name]), f"{time.time() - t0:.2f} s", flush=True)
    with open(dst, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(records)} cases to {dst}")
