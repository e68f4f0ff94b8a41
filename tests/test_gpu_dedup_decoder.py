"""GPU: the decoder's frame-only work on distinct rows (include/a3r.h,
a3r_model_set_dedup_decoder).  decoder_embed and zero_convs[0..4] run on the distinct enc_norm rows / depth-prior tokens with the
bias-only epilogue and a gather-add pass makes each slot's sum; block 0 runs everything before its cross-attention product on each
side's distinct (image, prior) entries and the cross-attention reads them through image maps.  What is pinned here: with the switch on, every output, every fh2 site scale and statistic, the
sizing query and the dedup reports equal the switch off bit for bit, whichever of the two kinds repeats, in forward and encode +
decode, in every arithmetic mode and across two calls; block 0 merges exactly when a3r.h says so (fewer entries than slots, and
row counts without a partial row tile: 256x256 and 128x128 frames here, never 64x96 or 48x80); and the new kernels alone equal
the attention on gathered operands / torch's fp32 sum exactly.  TINY config, synthetic weights."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_view_arrays
from align3r_amd.weights import TINY, synthetic_state_dict

pytestmark = pytest.mark.gpu
KEYS = ("pts3d_1", "conf_1", "pts3d_2", "conf_2")


def _engine():
    from align3r_amd.engine import PairEngine
    return PairEngine(TINY, synthetic_state_dict(TINY, 0))


@pytest.fixture(scope="module")
def eng():
    return _engine()


@pytest.fixture(scope="module")
def pool():
    """10 frames at 64x96 (N = 24 tokens), made once and left unchanged"""
    v = make_view_arrays(10, 64, 96, 3)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


@pytest.fixture(scope="module")
def pool_odd():
    """4 frames at 48x80: N = 15 tokens, odd row counts everywhere"""
    v = make_view_arrays(4, 48, 80, 5)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


@pytest.fixture(scope="module")
def pool256():
    """5 frames at 256x256: N = 256 tokens, so that every row count is a whole number of 256-row tiles"""
    v = make_view_arrays(5, 256, 256, 7)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


@pytest.fixture(scope="module")
def pool128():
    """4 frames at 128x128: N = 64 tokens, whole tiles with B and Um multiples of 4"""
    v = make_view_arrays(4, 128, 128, 9)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


def batch(items, idx):
    return torch.stack([items[i] for i in idx]).contiguous()


def record(e, run, phase):
    out = {k: t.clone() for k, t in run().items()}
    return out, e.site_scales(phase).copy(), e.site_stats().copy(), e.last_dedup(), e.last_dedup_sides()


def on_and_off(e, run, B, H, W, want_dedup=None, want_entries=None, phase=0, mode=1, sites=True):
    """the switch off, then on, from the same carried scales: equal bits everywhere; returns the off state's outputs"""
    try:
        e.set_dedup(mode)
        run()                                        # settles the range scales, so that both states start from the same ones
        e.set_dedup_decoder(False)
        ws_off = e.workspace_bytes(B, H, W)
        off = record(e, run, phase)
        assert e.last_dedup_entries() == (B, B, False)
        e.set_dedup_decoder(True)
        ws_on = e.workspace_bytes(B, H, W)
        on = record(e, run, phase)
        assert e.last_dedup_entries() == (want_entries if want_entries is not None else (B, B, False)), e.last_dedup_entries()
    finally:
        e.set_dedup(1)
        e.set_dedup_decoder(True)
    assert ws_on == ws_off
    for k in KEYS:
        assert torch.equal(on[0][k], off[0][k]), k
    assert on[1].shape == off[1].shape and np.array_equal(on[1], off[1])
    assert on[2].shape == off[2].shape and np.array_equal(on[2], off[2])
    assert (on[2] > 0).any() if sites else on[2].size == 0      # (only the fh2 forms have sites)
    assert on[3] == off[3] and on[4] == off[4]
    if want_dedup is not None:
        assert on[3] == want_dedup, on[3]
    return off[0]


def fwd(e, img, pd, i1, i2, d1=None, d2=None, **kw):
    args = (batch(img, i1), batch(img, i2), batch(pd, i1 if d1 is None else d1), batch(pd, i2 if d2 is None else d2))
    H, W = args[0].shape[-2:]
    return on_and_off(e, lambda: e.forward(*args), len(i1), H, W, **kw)


def test_chain_frames_on_both_sides(eng, pool, pool256):
    fwd(eng, *pool256, [0, 1, 2, 0, 1], [1, 2, 3, 1, 2], want_dedup=(4, 4, False), want_entries=(3, 3, True))
    fwd(eng, *pool, [0, 1, 2, 0, 1], [1, 2, 3, 1, 2], want_dedup=(4, 4, False), want_entries=(3, 3, False))      # 5 x 24 rows: a partial tile


def test_as_many_entries_as_slots_keep_block_0_per_slot(eng, pool):
    """U = B on a side: level 0 and the zero-convs still run on distinct rows"""
    fwd(eng, *pool, [0, 1, 2], [1, 2, 3], want_dedup=(4, 4, False), want_entries=(3, 3, False))
    fwd(eng, *pool, [0, 0, 0], [1, 2, 3], want_dedup=(4, 4, False), want_entries=(1, 3, False))


def test_fan_one_frame_on_a_side(eng, pool, pool256):
    """U_0 = 1, U_1 = 3: side 0's list is padded with copies of its entry"""
    fwd(eng, *pool256, [0, 0, 0, 0], [1, 2, 3, 1], want_dedup=(4, 4, False), want_entries=(1, 3, True))
    fwd(eng, *pool256, [1, 2, 3, 1], [0, 0, 0, 0], want_dedup=(4, 4, False), want_entries=(3, 1, True))
    fwd(eng, *pool, [0, 0, 0, 0], [1, 2, 3, 1], want_dedup=(4, 4, False), want_entries=(1, 3, False))


def test_five_pairs_sides_swapped(eng, pool, pool256):
    fwd(eng, *pool256, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(3, 3, False), want_entries=(3, 3, True))
    fwd(eng, *pool, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(3, 3, False), want_entries=(3, 3, False))


def test_whole_row_tiles_decide(eng, pool128):
    """N = 64: 8 slots and 4 entries per side are whole 256-row tiles, 3 entries are not"""
    fwd(eng, *pool128, [0, 1, 2, 3, 0, 1, 2, 3], [1, 2, 3, 0, 1, 2, 3, 0], want_dedup=(4, 4, False), want_entries=(4, 4, True))
    fwd(eng, *pool128, [0, 1, 2, 0, 1, 2, 0, 1], [1, 2, 0, 1, 2, 0, 1, 2], want_dedup=(3, 3, False), want_entries=(3, 3, False))
    fwd(eng, *pool128, [0, 1, 2, 3, 0, 1], [1, 2, 3, 0, 1, 2], want_dedup=(4, 4, False), want_entries=(4, 4, False))      # 6 slots


def test_only_one_kind_repeats(eng, pool):
    """repeated images with every prior distinct: the plain level 0 and zero-convs; repeated priors with every image distinct: the
    zero-convs on distinct rows, level 0 through the same path"""
    i1, i2 = [0, 0, 1, 2, 1], [1, 2, 0, 0, 2]
    d1, d2 = list(range(5)), list(range(5, 10))
    fwd(eng, *pool, i1, i2, d1=d1, d2=d2, want_dedup=(3, 10, False))
    fwd(eng, *pool, d1, d2, d1=i1, d2=i2, want_dedup=(10, 3, False))


def test_an_image_with_two_priors_and_a_prior_with_two_images(eng, pool, pool256):
    """the level-0 sum takes its two rows through two different maps"""
    fwd(eng, *pool, [0, 0, 1, 2], [1, 1, 2, 0], d1=[0, 1, 1, 2], d2=[3, 0, 0, 0], want_dedup=(3, 4, False), want_entries=(4, 4, False))
    # two images and two priors in three pairings per side: the entry is the pair
    fwd(eng, *pool256, [0, 0, 0, 1, 1], [1, 1, 1, 1, 0], d1=[0, 1, 0, 1, 1], d2=[1, 1, 0, 0, 0], want_dedup=(2, 2, False),
        want_entries=(3, 3, True))


def test_nothing_repeats(eng, pool):
    fwd(eng, *pool, [0, 1, 2], [3, 4, 5], want_dedup=(6, 6, False))


def test_odd_row_counts(eng, pool_odd):
    fwd(eng, *pool_odd, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(3, 3, False), want_entries=(3, 3, False))
    fwd(eng, *pool_odd, [2, 2, 2, 2], [0, 1, 0, 1], want_dedup=(3, 3, False), want_entries=(1, 2, False))
    fwd(eng, *pool_odd, [3], [3], want_dedup=(1, 1, False), want_entries=(1, 1, False))


def test_a_key_collision_runs_the_plain_plan(eng, pool256):
    fwd(eng, *pool256, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(10, 10, True), mode=2)


def test_a_tap_level_runs_the_plain_plan(pool256):
    e = _engine()
    e.set_tap_level(1)
    fwd(e, *pool256, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(10, 10, False))


def test_the_first_attention_form_runs_block_0_per_slot(eng, pool256):
    """a3r_attention_fh2_set_form(1): that kernel takes no image maps"""
    from align3r_amd import _lib
    lib = _lib.load()
    assert lib.a3r_attention_fh2_set_form(1) == 2
    try:
        fwd(eng, *pool256, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(3, 3, False))
    finally:
        assert lib.a3r_attention_fh2_set_form(2) == 1


def test_encode_and_decode_with_equal_feature_rows(eng, pool):
    img, pd = pool
    i1, i2 = [0, 1, 2, 0], [1, 2, 3, 3]
    f = eng.encode(batch(img, [0, 1, 2, 3]))
    f1, f2, d1, d2 = batch(f, i1), batch(f, i2), batch(pd, i1), batch(pd, i2)
    ref = on_and_off(eng, lambda: eng.decode(f1, f2, d1, d2, 64, 96), 4, 64, 96, want_dedup=(8, 4, False), phase=2)
    whole = eng.forward(batch(img, i1), batch(img, i2), d1, d2)
    for k in KEYS:
        assert torch.equal(whole[k], ref[k]), k


@pytest.mark.parametrize("gemm", ["f16", "bf3", "f32"])
def test_the_other_arithmetic_modes(monkeypatch, gemm, pool256):
    """one-pass fh2 takes the same path; bf3 and f32 keep the plain plan"""
    monkeypatch.setenv("A3R_GEMM", gemm)
    fwd(_engine(), *pool256, [0, 0, 1, 2, 1], [1, 2, 0, 0, 2], want_dedup=(3, 3, False), want_entries=(3, 3, True) if gemm == "f16" else None,
        sites=gemm == "f16")


def test_two_consecutive_calls_carry_the_same_scales(pool256):
    """from reset scales: two calls with the switch off against two with it on, on two engines of the same weights"""
    img, pd = pool256
    i1, i2, j1, j2 = [0, 1, 2, 0], [1, 2, 3, 1], [4, 4, 0, 4], [0, 3, 4, 0]
    a1 = (batch(img, i1), batch(img, i2), batch(pd, i1), batch(pd, i2))
    a2 = (batch(img, j1), batch(img, j2), batch(pd, j1), batch(pd, j2))
    res = {}
    for on in (False, True):
        e = _engine()
        e.set_dedup_decoder(on)
        res[on] = [record(e, lambda: e.forward(*a), 0) for a in (a1, a2)] + [e.range_reruns]
        assert e.last_dedup_entries() == ((2, 3, True) if on else (4, 4, False))
    assert res[True][2] == res[False][2]
    for r_on, r_off in zip(res[True][:2], res[False][:2]):
        for k in KEYS:
            assert torch.equal(r_on[0][k], r_off[0][k]), k
        assert np.array_equal(r_on[1], r_off[1]) and np.array_equal(r_on[2], r_off[2])
        assert r_on[3] == r_off[3] and r_on[4] == r_off[4]


def test_the_environment_sets_the_default(monkeypatch, pool):
    img, pd = pool
    args = (batch(img, [0, 1, 2]), batch(img, [1, 2, 3]), batch(pd, [0, 1, 2]), batch(pd, [1, 2, 3]))
    ref = {k: t.clone() for k, t in _engine().forward(*args).items()}
    monkeypatch.setenv("A3R_DEDUP_DEC", "0")
    off = _engine().forward(*args)
    for k in KEYS:
        assert torch.equal(off[k], ref[k]), k


# ---- the kernels alone
p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("N", [15, 24, 70])            # ragged against the 64-key tile and the 128-query block
@pytest.mark.parametrize("qi,ki", [([0, 1, 2], [0, 1, 2]), ([1, 1, 0], [3, 0, 3]), ([2, 0, 0], [1, 1, 1])])
def test_mapped_attention_equals_attention_on_gathered_operands(N, qi, ki, passes):
    """B = 3 batches, H = 2 heads; q images from a pool of 3, k / v images from a pool of 4 inside a wider k|v matrix"""
    from align3r_amd import _lib, ops
    B, H, Uq, Uk = 3, 2, 3, 4
    g = torch.Generator(device="cuda").manual_seed(N * 100 + sum(qi) * 10 + sum(ki))
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    q, kv = rnd(Uq, N, H * 64) * 2, rnd(Uk, N, 2 * H * 64) * 2
    qm, km = torch.tensor(qi, dtype=torch.int32, device="cuda"), torch.tensor(ki, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    lib.a3r_fh2_set_passes(passes)
    try:
        q2, kv2 = ops.split_fh2(q, 2.0), ops.split_fh2(kv, 0.5)
        w_ref = ops.absmax_word("cuda")
        qg, kvg = ops.split_fh2(q[qm.long()].contiguous(), 2.0), ops.split_fh2(kv[km.long()].contiguous(), 0.5)
        want = ops.attention_fh2(qg, kvg, kvg, B, H, N, N, v_col=H * 64, out_scale=4.0, out_absmax=w_ref)
        word = ops.absmax_word("cuda")
        o = torch.full((B * N * H * 64 * 4 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        r = _lib.Fh2AttnRange(2.0, 0.5, 0.5, 4.0, word.data_ptr())
        args = lambda out, a, b: (C.c_void_p(q2.data_ptr()), H * 64, C.c_void_p(kv2.data_ptr()), 2 * H * 64,
                                  C.c_void_p(kv2.data_ptr() + H * 64 * 4), 2 * H * 64, p(out), H * 64, B, H, N, N, C.byref(r), a, b,
                                  _lib.stream_ptr())
        assert lib.a3r_attention_fh2_mapped(*args(o, p(qm), p(km))) == 0
        assert torch.equal(o[:-16], want.data) and (o[-16:] == 0xA5).all()
        assert int(word.item()) == int(w_ref.item()) and int(word.item()) != 0
        if qi == ki:                                   # the identity: null maps are the same call
            o0 = torch.zeros_like(o)
            assert lib.a3r_attention_fh2_mapped(*args(o0, None, None)) == 0
            assert torch.equal(o0[:-16], want.data)
    finally:
        lib.a3r_fh2_set_passes(3)


@pytest.mark.parametrize("S,Ua,Ub,N,Cc,ia,ib", [
    (1, 1, 1, 1, 4, [0], [0]),                          # one float4
    (3, 2, 3, 15, 128, [1, 1, 0], [2, 0, 2]),
    (6, 4, 2, 24, 128, [0, 1, 2, 1, 2, 3], [0, 0, 1, 1, 0, 1]),
    (4, 2, 3, 5000, 68, [1, 0, 0, 1], [2, 2, 1, 0]),    # a row block that is no multiple of a workgroup
    (4, 2, 1, 22000, 768, [1, 0, 0, 1], [0, 0, 0, 0]),  # 16.9 M float4: more than the capped grid holds threads (65536 x 256)
])
def test_gather_add_rows_equals_torch(S, Ua, Ub, N, Cc, ia, ib):
    from align3r_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(S * 1000 + N)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g) * 3
    a, b, x = rnd(Ua, N, Cc), rnd(Ub, N, Cc), rnd(S, N, Cc)
    ma = torch.tensor(ia, dtype=torch.int32, device="cuda")
    mb = torch.tensor(ib, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    dst = torch.full((S, N, Cc), float("nan"), device="cuda")
    assert lib.a3r_gather_add_rows(p(a), p(ma), p(b), p(mb), p(dst), S, N, Cc, _lib.stream_ptr()) == 0
    assert torch.equal(dst, b[mb.long()] + a[ma.long()])
    dst = x.clone()
    assert lib.a3r_gather_add_rows(p(a), p(ma), None, None, p(dst), S, N, Cc, _lib.stream_ptr()) == 0
    assert torch.equal(dst, x + a[ma.long()])
