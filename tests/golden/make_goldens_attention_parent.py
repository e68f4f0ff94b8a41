"""Writes attention_parent.json: what the attention kernels (csrc/attention.hip exact fp32, attention_bf3.hip three-plane bf16,
attention_fh2.hip two-plane fp16 in both forms and the single-pass mode) compute, as the library selected by A3R_LIB (default: the
tree's own) computes it on the GPU.  The committed file pins the results of the commit BEFORE the kernels' placement, softmax step,
product ladders, staged operands, epilogue, entry checks and launch were shared (csrc/attention_tile.h):

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_attention_parent.py [--out FILE]

A case is one (kernel family, shape or group count); its record maps every launch of the case to the SHA-256 of the raw bytes of
the output and, for fh2 launches, of the out_absmax word.  The kernels take no floating-point atomics and the statistic is an
integer maximum, so a record is the same in every run.  Inputs are the seeded families of tests/attention_refs.py (assemble /
launch_groups: ten (batch, head) groups per launch, B = 2, H = 5), at most 10 x 257 query rows.

  f32/<Nq>x<Nk>       a3r_attention                                                                      every shape of SHAPES
  bf3/<Nq>x<Nk>       a3r_attention_bf3 with out_pair 0 and 1 (1 where ldo % 32 == 0) and a3r_attention_bf3_fh2out, each at
                      a3r_bf3_set_products 6 / 3 / 1                                                     every shape of SHAPES
  fh2/<Nq>x<Nk>       a3r_attention_fh2 in form 2 and form 1, at scale 1 and at the scaled set SCALED    every shape of SHAPES
  single/<Nq>x<Nk>    a3r_fh2_set_passes(1), form 2                                                      SINGLE_PASS_SHAPES
  mapped/<Nq>x<Nk>    a3r_attention_fh2_mapped, form 2, q_map = [1, 0] and kv_map = [1, 1]               LAYOUT_SHAPES
  sliced/<Nq>x<Nk>    q, k, v as column slices of one fused matrix: fp32, bf3, fh2 in both forms         LAYOUT_SHAPES
  groups/<B>x<H>      fp32, bf3 (both layouts), fh2 in both forms                                        GROUP_COUNTS on GROUP_SHAPE

Every process-wide mode (kernel form, products, passes) is put back in a `finally`.
tests/test_gpu_attention_parent.py imports CASES and measure_case() from here, so the test and the golden cannot drift apart."""
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

import attention_refs as R      # noqa: E402

B0, H0 = R.LAUNCH_B, R.LAUNCH_H
# the scaled launch of tests/test_gpu_attention_f64.py (SCALED_MUL, SCALED): q, k x 2^-6 stored at 2^6, v x 2^-10 stored at 2^10,
# the output written at 2^10
SCALED_MUL, SCALED = (2.0 ** -6, 2.0 ** -6, 2.0 ** -10), (2.0 ** 6, 2.0 ** 6, 2.0 ** 10, 2.0 ** 10)
Q_MAP, KV_MAP = (1, 0), (1, 1)

_tag = lambda s: f"{s[0]}x{s[1]}"
CASES = {}
for _s in R.SHAPES:
    for _k in ("f32", "bf3", "fh2"):
        CASES[f"{_k}/{_tag(_s)}"] = dict(kind=_k, shape=_s, groups=(B0, H0))
for _s in R.SINGLE_PASS_SHAPES:
    CASES[f"single/{_tag(_s)}"] = dict(kind="single", shape=_s, groups=(B0, H0))
for _s in R.LAYOUT_SHAPES:
    for _k in ("mapped", "sliced"):
        CASES[f"{_k}/{_tag(_s)}"] = dict(kind=_k, shape=_s, groups=(B0, H0))
for _g in R.GROUP_COUNTS:
    CASES[f"groups/{_tag(_g)}"] = dict(kind="groups", shape=R.GROUP_SHAPE, groups=_g)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.data if not hasattr(t, "cpu") else t          # ops.Bf3 / ops.Fh2 -> their storage
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


class _Mode:
    """with _Mode(setter, value): a process-wide mode for the block; the previous one is put back"""

    def __init__(self, setter, value):
        self.setter, self.value = setter, value

    def __enter__(self):
        self.prev = self.setter(self.value)

    def __exit__(self, *exc):
        self.setter(self.prev)


def _form(n):
    from align3r_amd import _lib
    return _Mode(_lib.load().a3r_attention_fh2_set_form, n)


def _inputs(case, mul=(1.0, 1.0, 1.0)):
    (Nq, Nk), (B, H) = case["shape"], case["groups"]
    q, k, v, _ = R.assemble(R.launch_groups(R.SHAPES.index((Nq, Nk)), B * H), B, H, Nq, Nk, mul)
    return _dev(q), _dev(k), _dev(v)


def _fused(q, k, v, B, Nq, Nk):
    """[B max(Nq, Nk), 3 D] with q, k, v as column blocks; q fills the first B Nq rows"""
    import torch
    D = q.shape[1]
    m = torch.zeros(B * max(Nq, Nk), 3 * D, device="cuda")
    m[:B * Nq, :D] = q
    m[:B * Nk, D:2 * D] = k
    m[:B * Nk, 2 * D:] = v
    return m


def _f32(q, k, v, B, H, Nq, Nk, ld=None, cols=(0, 0, 0)):
    import torch
    from align3r_amd import _lib
    D = H * 64
    ld = ld or D
    o = torch.zeros((B * Nq, D), device="cuda")
    p = lambda t, c=0: C.c_void_p(t.data_ptr() + 4 * c)
    _lib.check(_lib.load().a3r_attention(p(q, cols[0]), ld, p(k, cols[1]), ld, p(v, cols[2]), ld, p(o), D, B, H, Nq, Nk, _lib.stream_ptr()),
               "attention")
    return _sha(o)


def _bf3(rec, name, q3, k3, v3, B, H, Nq, Nk, fh2out=True, **cols):
    from align3r_amd import ops
    rec[f"{name}/plain"] = _sha(ops.attention_bf3(q3, k3, v3, B, H, Nq, Nk, **cols))
    if (H * 64) % 32 == 0:
        rec[f"{name}/pair"] = _sha(ops.attention_bf3(q3, k3, v3, B, H, Nq, Nk, out_pair=True, **cols))
    if fh2out:
        rec[f"{name}/fh2out"] = _sha(ops.attention_bf3_fh2out(q3, k3, v3, B, H, Nq, Nk, **cols))


def _fh2(rec, name, q2, k2, v2, B, H, Nq, Nk, out_scale=1.0, forms=(2, 1), **cols):
    from align3r_amd import ops
    for n in forms:
        with _form(n):
            word = ops.absmax_word("cuda")
            o2 = ops.attention_fh2(q2, k2, v2, B, H, Nq, Nk, out_scale=out_scale, out_absmax=word, **cols)
        rec[f"{name}/form{n}"], rec[f"{name}/form{n}/absmax"] = _sha(o2), _sha(word)


def _mapped(rec, q2, k2, v2, B, H, Nq, Nk):
    import torch
    from align3r_amd import _lib, ops
    D = H * 64
    qm, km = _dev(np.array(Q_MAP, np.int32)), _dev(np.array(KV_MAP, np.int32))
    word = ops.absmax_word("cuda")
    o = torch.zeros(B * Nq * D * 4, dtype=torch.uint8, device="cuda")
    r = _lib.Fh2AttnRange(1.0, 1.0, 1.0, 1.0, word.data_ptr())
    p = lambda t: C.c_void_p(t.data_ptr())
    with _form(2):
        _lib.check(_lib.load().a3r_attention_fh2_mapped(p(q2), D, p(k2), D, p(v2), D, p(o), D, B, H, Nq, Nk, C.byref(r), p(qm), p(km),
                                                        _lib.stream_ptr()), "attention_fh2_mapped")
    rec["form2"], rec["form2/absmax"] = _sha(o), _sha(word)


def measure_case(name):
    """the record of one case from the loaded library"""
    from align3r_amd import ops
    case = CASES[name]
    kind, (Nq, Nk), (B, H) = case["kind"], case["shape"], case["groups"]
    D = H * 64
    assert B * Nq <= 10 * 257
    rec = {}
    with _Mode(ops.bf3_set_products, 6), _Mode(ops.fh2_set_passes, 3):          # the default modes, whatever ran before
        q, k, v = _inputs(case)
        if kind == "f32":
            rec["out"] = _f32(q, k, v, B, H, Nq, Nk)
        elif kind == "bf3":
            q3, k3, v3 = ops.split_bf3(q), ops.split_bf3(k), ops.split_bf3(v)
            for np_ in (6, 3, 1):
                with _Mode(ops.bf3_set_products, np_):
                    _bf3(rec, f"products{np_}", q3, k3, v3, B, H, Nq, Nk)
        elif kind == "fh2":
            _fh2(rec, "scale1", ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B, H, Nq, Nk)
            qs, ks, vs, os_ = SCALED
            q, k, v = _inputs(case, SCALED_MUL)
            _fh2(rec, "scaled", ops.split_fh2(q, qs), ops.split_fh2(k, ks), ops.split_fh2(v, vs), B, H, Nq, Nk, out_scale=os_)
        elif kind == "single":
            q2, k2, v2 = ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v)
            with _Mode(ops.fh2_set_passes, 1):
                _fh2(rec, "passes1", q2, k2, v2, B, H, Nq, Nk, forms=(2,))
        elif kind == "mapped":
            _mapped(rec, ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B, H, Nq, Nk)
        elif kind == "sliced":
            qkv = _fused(q, k, v, B, Nq, Nk)
            cols = dict(q_col=0, k_col=D, v_col=2 * D)
            rec["f32"] = _f32(qkv, qkv, qkv, B, H, Nq, Nk, ld=3 * D, cols=(0, D, 2 * D))
            qkv3, qkv2 = ops.split_bf3(qkv), ops.split_fh2(qkv)
            _bf3(rec, "bf3", qkv3, qkv3, qkv3, B, H, Nq, Nk, **cols)
            _fh2(rec, "fh2", qkv2, qkv2, qkv2, B, H, Nq, Nk, **cols)
        else:
            assert kind == "groups"
            rec["f32"] = _f32(q, k, v, B, H, Nq, Nk)
            _bf3(rec, "bf3", ops.split_bf3(q), ops.split_bf3(k), ops.split_bf3(v), B, H, Nq, Nk, fh2out=False)
            _fh2(rec, "fh2", ops.split_fh2(q), ops.split_fh2(k), ops.split_fh2(v), B, H, Nq, Nk)
    return rec


if __name__ == "__main__":
    dst = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(HERE, "attention_parent.json")
    records = {}
    for name in CASES:
        records[name] = measure_case(name)
        print(name, "ok", len(records[name]), flush=True)
    with open(dst, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(records)} cases to {dst}")
