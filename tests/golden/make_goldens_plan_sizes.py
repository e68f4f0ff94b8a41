"""Writes plan_sizes.json: the packed-buffer and workspace sizes of the pair network and the flow network for a grid of configs,
arithmetic modes and shapes, as the library selected by A3R_LIB (default: the tree's own) reports them.  The sizing passes run on
the host, no GPU needed.  The committed file pins the sizes of the commit BEFORE the launch-plan core was shared (csrc/plan.h):

    A3R_LIB=/path/to/that/commit/liba3r.so python tests/golden/make_goldens_plan_sizes.py

tests/test_plan_sizes_cpu.py imports measure() from here, so the test and the golden cannot drift apart."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (A3R_GEMM, A3R_CONV); None = unset.  Both are read by a3r_model_create.
MODES = {"unset": (None, None), "f32": ("f32", None), "bf3": ("bf3", None), "bf3x3": ("bf3x3", None), "bf16": ("bf16", None),
         "f16": ("f16", None), "unset+conv_bf3": (None, "bf3")}
MODEL_SHAPES = [(1, 48, 80), (2, 64, 96), (3, 48, 80), (1, 512, 288), (42, 384, 512)]      # odd and even row counts: pair mode
# (1, 136, 168): an odd 17 x 21 eighth-resolution map, so every pyramid level is a floor
RAFT_SHAPES = [(1, 128, 128), (2, 136, 160), (12, 384, 512), (3, 128, 160), (1, 136, 168), (48, 288, 512)]


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def measure():
    """{case: sizes} from the loaded library."""
    from align3r_amd import _lib
    from align3r_amd.weights import TINY, VITL
    from align3r_amd.raft_weights import RAFT_M, RAFT_TINY
    lib = _lib.load()
    out = {}
    saved = {k: os.environ.get(k) for k in ("A3R_GEMM", "A3R_CONV")}
    try:
        for cname, cfg in (("TINY", TINY), ("VITL", VITL)):
            c = _lib.ModelConfigC(cfg.enc_embed_dim, cfg.enc_depth, cfg.enc_num_heads, cfg.dec_embed_dim, cfg.dec_depth, cfg.dec_num_heads,
                                  cfg.mlp_ratio, cfg.patch_size, cfg.rope_base, cfg.feature_dim, cfg.last_dim, (C.c_int * 4)(*cfg.layer_dims))
            for mname, (gemm, conv) in MODES.items():
                _setenv("A3R_GEMM", gemm)
                _setenv("A3R_CONV", conv)
                h = C.c_void_p()
                _lib.check(lib.a3r_model_create(C.byref(c), C.byref(h)), "a3r_model_create")
                out[f"model/{cname}/{mname}/packed"] = lib.a3r_model_packed_bytes(h)
                for B, H, W in MODEL_SHAPES:
                    out[f"model/{cname}/{mname}/{B}x{H}x{W}/workspace"] = lib.a3r_model_workspace_bytes(h, B, H, W)
                    out[f"model/{cname}/{mname}/{B}x{H}x{W}/encode_workspace"] = lib.a3r_model_encode_workspace_bytes(h, B, H, W)
                _lib.check(lib.a3r_model_destroy(h))
    finally:
        for k, v in saved.items():
            _setenv(k, v)
    for cname, cfg in (("tiny", RAFT_TINY), ("full", RAFT_M)):
        c = _lib.RaftConfigC(cfg.initial_dim, (C.c_int * 3)(*cfg.block_dims), (C.c_int * 3)(*cfg.n_blocks), cfg.dim, cfg.radius,
                             cfg.corr_levels, cfg.num_blocks)
        h = C.c_void_p()
        _lib.check(lib.a3r_raft_create(C.byref(c), C.byref(h)), "a3r_raft_create")
        out[f"raft/{cname}/packed"] = lib.a3r_raft_packed_bytes(h)
        for B, H, W in RAFT_SHAPES:
            out[f"raft/{cname}/{B}x{H}x{W}/workspace"] = lib.a3r_raft_workspace_bytes(h, B, H, W)
        _lib.check(lib.a3r_raft_destroy(h))
    return out


if __name__ == "__main__":
    sizes = measure()
    assert all(v > 0 for v in sizes.values()), [k for k, v in sizes.items() if v <= 0]
    with open(os.path.join(HERE, "plan_sizes.json"), "w") as f:
        json.dump(sizes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(sizes)} sizes")
