"""GPU: the DPT heads run their level-0 branch (adapter, 4x transposed conv, layer_rn[0], the two convs of refinenet1.resConfUnit1)
once per DISTINCT frame of their side and a combine pass puts the rows back (include/a3r.h, a3r_model_set_dedup_head).  What is
pinned here: with the head merge on, every output equals the head merge off and dedup mode 0 bit for bit; the two sides merge
separately and only when a3r.h says so (fewer distinct frames than slots, inside the admission bound, fh2 maps, no fallback); the fh2
sites, scales, statistics and range re-runs are the same; decode merges on equal feature rows; and the combine kernel alone equals
torch's fp32 c[map] + (r0[map] + p2) and the split of its ReLU.  TINY config, synthetic weights."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_view_arrays
from align3r_amd.weights import TINY, synthetic_state_dict

pytestmark = pytest.mark.gpu
KEYS = ("pts3d_1", "conf_1", "pts3d_2", "conf_2")
I1, I2 = [0, 0, 1, 2, 1], [1, 2, 0, 0, 2]         # B = 5 from 3 frames, sides swapped


def _engine(sd=None):
    from align3r_amd.engine import PairEngine
    return PairEngine(TINY, sd if sd is not None else synthetic_state_dict(TINY, 0))


@pytest.fixture(scope="module")
def eng():
    return _engine()


@pytest.fixture(scope="module")
def pool():
    """20 frames at 64x96, made once and left unchanged"""
    v = make_view_arrays(20, 64, 96, 3)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


def frames(n, H, W, seed=3):
    v = make_view_arrays(n, H, W, seed)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


def batch(items, idx):
    return torch.stack([items[i] for i in idx]).contiguous()


def fits(B, U, N, cfg=TINY):
    """The admission rule of a3r.h, from the buffer sizes: the level-0 buffers of the merged branch (a0, l0, its fh2 form, r0, its
    fh2 form on U images, plus the compact enc_norm rows and the bias-only conv output) fit what the plain plan reserves for the
    first five on B images; every buffer rounded up to 256 bytes."""
    l, F, E = cfg.layer_dims[0], cfg.feature_dim, cfg.enc_embed_dim
    size = lambda n, per: sum((n * N * p * 4 + 255) // 256 * 256 for p in per)
    plain = [l, 16 * l, 16 * l, 16 * F, 16 * F]
    return 0 < U < B and size(U, plain + [E, 16 * F]) <= size(B, plain)


def three_ways(run, e, B, want_sides, want_dedup=None, mode=1):
    """dedup mode 0, mode `mode` with the head merge off, and with it on: equal bits on all four outputs; returns mode 0's."""
    try:
        e.set_dedup(0)
        ref = {k: t.clone() for k, t in run().items()}
        assert e.last_dedup_sides() == (B, B, False, False)
        e.set_dedup(mode)
        e.set_dedup_head(False)
        off = {k: t.clone() for k, t in run().items()}
        assert e.last_dedup_sides() == (B, B, False, False)
        e.set_dedup_head(True)
        on = run()
        assert e.last_dedup_sides() == want_sides, e.last_dedup_sides()
        if want_dedup is not None:
            assert e.last_dedup() == want_dedup, e.last_dedup()
        for k in KEYS:
            assert torch.equal(off[k], ref[k]), k
            assert torch.equal(on[k], ref[k]), k
    finally:
        e.set_dedup(1)
        e.set_dedup_head(True)
    return ref


def fwd3(e, img, pd, i1, i2, want_sides, d1=None, d2=None, **kw):
    args = (batch(img, i1), batch(img, i2), batch(pd, i1 if d1 is None else d1), batch(pd, i2 if d2 is None else d2))
    return three_ways(lambda: e.forward(*args), e, len(i1), want_sides, **kw)


def test_both_sides_merge(eng, pool):
    assert fits(5, 3, 24)
    fwd3(eng, *pool, I1, I2, (3, 3, True, True), want_dedup=(3, 3, False))


def test_the_sides_decide_separately(eng, pool):
    """side 1 all one frame, side 2 all distinct"""
    fwd3(eng, *pool, [0, 0, 0, 0], [1, 2, 3, 4], (1, 4, True, False))
    fwd3(eng, *pool, [1, 2, 3, 4], [0, 0, 0, 0], (4, 1, False, True))


def test_admission_bound(eng, pool):
    """B = 10, N = 24, TINY (l = 96, F = 256, E = 128): U (33 l + 48 F + E) <= B (33 l + 32 F) gives U <= 0.729 B, so 7 distinct
    frames merge and 8 do not; nor does B - 1."""
    B, N = 10, 24
    assert fits(B, 7, N) and not fits(B, 8, N) and not fits(B, 9, N)
    side = lambda U: list(range(U)) + [0] * (B - U)
    other = [10 + i for i in range(B)]                  # all distinct, and none of them on the first side
    for U in (7, 8, 9):
        fwd3(eng, *pool, side(U), other, (U, B, fits(B, U, N), False))
    fwd3(eng, *pool, other, side(7), (B, 7, False, True))


def test_only_repeated_images_merge_the_head(eng, pool):
    d1, d2 = list(range(5)), list(range(5, 10))
    fwd3(eng, *pool, I1, I2, (3, 3, True, True), d1=d1, d2=d2, want_dedup=(3, 10, False))        # every depth prior distinct
    img, pd = pool
    args = (batch(img, d1), batch(img, d2), batch(pd, I1), batch(pd, I2))                        # every image distinct
    three_ways(lambda: eng.forward(*args), eng, 5, (5, 5, False, False), want_dedup=(10, 3, False))


def test_odd_row_counts_and_cropped_maps(eng):
    """48x80: N = 15 tokens per frame, 3 x 5 patches -- odd row counts everywhere, and 256-byte rounding enters the bound"""
    img, pd = frames(3, 48, 80)
    ok = fits(5, 3, 15)
    fwd3(eng, img, pd, I1, I2, (3, 3, ok, ok))
    ok = fits(4, 1, 15)
    fwd3(eng, img, pd, [2, 2, 2, 2], [0, 1, 0, 2], (1, 3, ok, fits(4, 3, 15)))


@pytest.mark.parametrize("gemm", ["fh2", "bf3", "f32"])
def test_every_arithmetic_mode(monkeypatch, gemm, pool):
    """the bf3 and f32 maps keep the plain head; the bits equal mode 0 in each"""
    monkeypatch.setenv("A3R_GEMM", gemm)
    e = _engine()
    fwd3(e, *pool, I1, I2, (3, 3, True, True) if gemm == "fh2" else (5, 5, False, False), want_dedup=(3, 3, False))


@pytest.mark.parametrize("fold", ["0", "1"])
def test_both_forms_of_the_combine_pass(monkeypatch, fold, pool):
    """A3R_DEDUP_HEAD_FOLD=0: the combine kernel after refinenet2's fp32 2x up-sample; 1 (default): inside that up-sample"""
    monkeypatch.setenv("A3R_DEDUP_HEAD_FOLD", fold)
    e = _engine()
    fwd3(e, *pool, I1, I2, (3, 3, True, True))
    fwd3(e, *pool, [0, 0, 0, 0], [1, 2, 3, 4], (1, 4, True, False))
    img, pd = frames(3, 48, 80)
    ok = fits(5, 3, 15)
    fwd3(e, img, pd, I1, I2, (3, 3, ok, ok))


def test_a_key_collision_runs_the_plain_head(eng, pool):
    fwd3(eng, *pool, I1, I2, (5, 5, False, False), want_dedup=(10, 10, True), mode=2)


def test_sites_scales_and_statistics(eng, pool):
    img, pd = pool
    args = (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2))
    res = {}
    try:
        for on in (False, True):
            eng.set_dedup_head(on)
            eng.forward(*args)
            res[on] = (eng.site_scales(0).copy(), eng.site_stats().copy(), eng.last_dedup_sides())
    finally:
        eng.set_dedup_head(True)
    assert res[True][2] == (3, 3, True, True) and res[False][2] == (5, 5, False, False)
    assert res[False][0].shape == res[True][0].shape and np.array_equal(res[False][0], res[True][0])
    assert res[False][1].shape == res[True][1].shape and np.array_equal(res[False][1], res[True][1])
    assert (res[True][1] > 0).any()


def test_range_control_repeats_equally(pool):
    """Weights scaled so that the level-0 sites leave their band on the first attempt (as test_gpu_dedup.py): from reset scales the
    merged and the plain head repeat equally often and end with the same scales and outputs."""
    sd = {k: np.array(v, copy=True) for k, v in synthetic_state_dict(TINY, 0).items()}
    heads = ("downstream_head1.dpt.", "downstream_head2.dpt.")
    for k in ("enc_norm.weight", "enc_norm.bias"):
        sd[k] = (sd[k] * np.float32(2.0 ** -20)).astype(np.float32)
    for k in ["decoder_embed.weight"] + [h + "act_postprocess.0.0.weight" for h in heads]:
        sd[k] = (sd[k] * np.float32(2.0 ** 20)).astype(np.float32)
    e = _engine(sd)
    img, pd = pool
    args = (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2))
    res = {}
    for on in (False, True):
        e.set_dedup_head(on)
        e.reset_ranges()
        n0 = e.range_reruns
        out = {k: t.clone() for k, t in e.forward(*args).items()}
        res[on] = (e.range_reruns - n0, e.site_scales(0).copy(), out, e.last_dedup_sides())
    assert res[False][0] >= 1 and res[True][0] == res[False][0]
    assert res[True][3] == (3, 3, True, True)
    assert np.array_equal(res[False][1], res[True][1])
    for k in KEYS:
        assert torch.equal(res[False][2][k], res[True][2][k]), k


def test_decode_merges_on_equal_feature_rows(eng, pool):
    img, pd = pool
    f = eng.encode(batch(img, [0, 1, 2]))
    f1, f2, d1, d2 = batch(f, I1), batch(f, I2), batch(pd, I1), batch(pd, I2)
    ref = three_ways(lambda: eng.decode(f1, f2, d1, d2, 64, 96), eng, 5, (3, 3, True, True), want_dedup=(10, 3, False))
    fwd = eng.forward(batch(img, I1), batch(img, I2), d1, d2)
    for k in KEYS:
        assert torch.equal(fwd[k], ref[k]), k


# ---- the combine kernel alone
@pytest.mark.parametrize("S,U,P,Cc,scale,idx", [
    (1, 1, 1, 8, 1.0, [0]),                        # one pixel, one 8-channel group
    (1, 1, 5, 32, 4.0, [0]),
    (3, 2, 7, 16, 0.5, [1, 1, 0]),
    (3, 3, 13, 256, 1.0, [2, 0, 1]),               # 39 pixel rows of 32 threads: no multiple of a workgroup's 8 rows
    (4, 2, 50000, 24, 2.0, [1, 0, 0, 1]),          # more work than the persistent grid holds; 3 threads per row do not divide its stride
])
def test_combine_kernel(S, U, P, Cc, scale, idx):
    from align3r_amd import _lib, ops
    g = torch.Generator(device="cuda").manual_seed(S * 1000 + P)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g) * 3
    c, r0, p2 = rnd(U, P, Cc), rnd(U, P, Cc), rnd(S, P, Cc)
    m = torch.tensor(idx, dtype=torch.int32, device="cuda")
    s = torch.full((S, P, Cc), float("nan"), device="cuda")
    sr2 = torch.zeros(S * P * Cc * 4, dtype=torch.uint8, device="cuda")
    word = ops.absmax_word("cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.load().a3r_combine_resid_fh2(p(c), p(r0), p(p2), p(m), p(s), p(sr2), S, P, Cc, scale, p(word), _lib.stream_ptr())
    assert rc == 0
    want = c[m.long()] + (r0[m.long()] + p2)
    assert torch.equal(s, want)
    assert want.numel() < 64 or ((want < 0).any() and (want > 0).any())
    w2 = ops.absmax_word("cuda")
    split = ops.split_fh2(torch.relu(want), scale, w2)
    assert torch.equal(sr2, split.data)
    assert int(word.item()) == int(w2.item())
    assert ops.absmax_value(word) == float((torch.relu(want) * scale).max())
