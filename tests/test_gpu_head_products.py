"""GPU: the head products a handle keeps across forward calls (include/a3r.h, a3r_model_set_head_products): the level-0 branch of a
DPT head -- adapter, 4x transposed conv, layer_rn[0], the two convs of refinenet1.resConfUnit1 -- runs only on those distinct frames
of a merging side whose (entry, side) bit is not set, and the combine pass reads the stored r0 and c in place.  What is pinned here
is that nothing else changes: every output equals, bit for bit, that of an engine built with head_products=False, whatever mixture
of stored and fresh frames a side holds; the report counts them per side; a frame stored for one side is a miss on the other; an
entry the frame cache refills loses both bits (stale rows would show as different outputs: the frames differ strongly); a frame
without an entry is computed and not stored; both forms of the combine pass; a side outside the admission bound neither reads nor
writes; the switches bypass it; everything that drops the frame cache drops it; range re-runs, scales and the statistics words of
a repeated batch are the plain handle's.  And the two source-indexed combine entry points alone against torch.
TINY config, synthetic weights, 64x96 and 48x80 (N = 24 and 15), B = 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_view_arrays
from align3r_amd.weights import TINY, synthetic_state_dict

pytestmark = pytest.mark.gpu
KEYS = ("pts3d_1", "conf_1", "pts3d_2", "conf_2")
NONE = ((0, 0), (0, 0))


def _engine(frame_cache, sd=None, **kw):
    from align3r_amd.engine import PairEngine
    return PairEngine(TINY, sd if sd is not None else synthetic_state_dict(TINY, 0), frame_cache=frame_cache, **kw)


@pytest.fixture()
def off():
    """the engine every output is compared with: the same storages but the head products (a new one per test, as the engine under
    test is: both then see the same calls)"""
    e = _engine(8, head_products=False)
    assert e._hp_store is None and not e.head_products
    return e


@pytest.fixture()
def eng():
    e = _engine(8)
    assert e.head_products
    return e


_frames = {}


def frames(H, W):
    """9 frames that differ strongly: frame i is scaled by 0.4 + 0.2 i"""
    if (H, W) not in _frames:
        v = make_view_arrays(9, H, W, seed=7)
        _frames[H, W] = ([torch.from_numpy(a[0][0] * np.float32(0.4 + 0.2 * i)).cuda() for i, a in enumerate(v)],
                         [torch.from_numpy(a[1][0]).cuda() for a in v])
    return _frames[H, W]


def args_of(img, pd, i1, i2):
    st = lambda items, idx: torch.stack([items[i] for i in idx]).contiguous()
    return st(img, i1), st(img, i2), st(pd, i1), st(pd, i2)


def run(e, args):
    return {k: t.clone() for k, t in e.forward(*args).items()}


def same(out, ref):
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k


def fits(B, U, N, cfg=TINY):
    """the admission rule of a3r.h (tests/test_gpu_dedup_head.py)"""
    l, F, E = cfg.layer_dims[0], cfg.feature_dim, cfg.enc_embed_dim
    size = lambda n, per: sum((n * N * p * 4 + 255) // 256 * 256 for p in per)
    plain = [l, 16 * l, 16 * l, 16 * F, 16 * F]
    return 0 < U < B and size(U, plain + [E, 16 * F]) <= size(B, plain)


def step(eng, off, args, want, sides=None):
    """one call on both engines: equal bits, and the report of the engine under test"""
    same(run(eng, args), run(off, args))
    assert eng.last_head_products() == want, eng.last_head_products()
    assert off.last_head_products() == NONE
    assert eng.last_dedup_sides() == off.last_dedup_sides()
    if sides is not None:
        assert eng.last_dedup_sides() == sides, eng.last_dedup_sides()
    assert eng.last_frame_cache() == off.last_frame_cache() and eng.last_frame_products() == off.last_frame_products()


A = ([0, 0, 1, 2, 1], [1, 2, 0, 0, 2])          # frames 0 1 2 on both sides, B = 5
B_ = ([2, 3, 2, 4, 3], [3, 2, 4, 2, 2])         # frames 2 3 4: 2 is old after A


def pair(a, b):
    """B = 5 from two frames, a b on side 1 and b a on side 2"""
    return [a, a, b, b, a], [b, b, a, a, b]


@pytest.mark.parametrize("hw", [(64, 96), (48, 80)])
def test_same_batch_twice(eng, off, hw):
    """the second call finds every frame of both sides and launches nothing of the branch (misses 0); the statistics words and
    scales are those of a handle without any storage, byte for byte"""
    img, pd = frames(*hw)
    N = (hw[0] // 16) * (hw[1] // 16)
    assert fits(5, 3, N)
    args = args_of(img, pd, *A)
    plain = _engine(0)
    ref = run(plain, args)
    assert plain.last_head_products() == NONE
    step(eng, off, args, ((0, 3), (0, 3)), sides=(3, 3, True, True))
    st1 = eng.site_stats()
    step(eng, off, args, ((3, 0), (3, 0)), sides=(3, 3, True, True))
    same(run(eng, args), ref)
    assert eng.last_head_products() == ((3, 0), (3, 0))
    st2 = eng.site_stats()
    want = plain.site_stats()
    assert (want > 0).any() and st1.tobytes() == want.tobytes() and st2.tobytes() == want.tobytes()
    assert eng.site_scales(0).tobytes() == plain.site_scales(0).tobytes()
    assert eng.range_reruns == plain.range_reruns


@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("hw", [(64, 96), (48, 80)])
def test_partial_overlap_in_both_forms_of_the_combine_pass(monkeypatch, fold, hw):
    """each side mixes stored and fresh frames; then all stored"""
    monkeypatch.setenv("A3R_DEDUP_HEAD_FOLD", fold)
    eng, off = _engine(8), _engine(8, head_products=False)
    img, pd = frames(*hw)
    step(eng, off, args_of(img, pd, *A), ((0, 3), (0, 3)))
    step(eng, off, args_of(img, pd, *B_), ((1, 2), (1, 2)), sides=(3, 3, True, True))
    # side 1: 0 3 1 all stored; side 2: 4 (stored by B_), 5 (new), 0 (stored by A)
    step(eng, off, args_of(img, pd, [0, 3, 0, 3, 1], [4, 4, 5, 0, 0]), ((3, 0), (2, 1)))
    step(eng, off, args_of(img, pd, *B_), ((3, 0), (3, 0)))
    step(eng, off, args_of(img, pd, *A), ((3, 0), (3, 0)))


def test_a_frame_stored_for_one_side_is_a_miss_on_the_other(eng, off):
    img, pd = frames(64, 96)
    assert fits(5, 2, 24)
    step(eng, off, args_of(img, pd, [0, 0, 1, 1, 0], [2, 3, 2, 3, 3]), ((0, 2), (0, 2)), sides=(2, 2, True, True))
    swapped = args_of(img, pd, [2, 2, 3, 3, 2], [0, 1, 0, 1, 1])
    step(eng, off, swapped, ((0, 2), (0, 2)))
    assert eng.last_frame_cache() == (4, 0, 0)              # the frames themselves were all found
    step(eng, off, swapped, ((2, 0), (2, 0)))
    step(eng, off, args_of(img, pd, [0, 0, 1, 1, 0], [2, 3, 2, 3, 3]), ((2, 0), (2, 0)))


def test_eviction_clears_both_sides():
    """4 entries, 8 frames taking turns two by two: every return of a pair finds its entries refilled by other frames"""
    eng, off = _engine(4), _engine(4, head_products=False)
    img, pd = frames(64, 96)
    for turn in range(2):
        for i in range(4):
            step(eng, off, args_of(img, pd, *pair(2 * i, 2 * i + 1)), ((0, 2), (0, 2)), sides=(2, 2, True, True))
            assert eng.last_frame_cache() == (0, 2, 2 if (turn or i >= 2) else 0)
    # frames 4 5 6 7 are the stored ones now: both sides of each
    step(eng, off, args_of(img, pd, *pair(6, 7)), ((2, 0), (2, 0)))
    step(eng, off, args_of(img, pd, *pair(4, 5)), ((2, 0), (2, 0)))
    # 0 replaces the least recently used entry (6's); 7 stays.  Then 6 comes back into another entry: a miss on both sides
    step(eng, off, args_of(img, pd, *pair(0, 7)), ((1, 1), (1, 1)))
    assert eng.last_frame_cache() == (1, 1, 1)
    step(eng, off, args_of(img, pd, *pair(6, 0)), ((1, 1), (1, 1)))
    step(eng, off, args_of(img, pd, *pair(6, 0)), ((2, 0), (2, 0)))


def test_more_fresh_frames_than_free_entries():
    """2 entries, 3 frames: the third is computed, read from the arena and not stored -- in every call"""
    eng, off = _engine(2), _engine(2, head_products=False)
    img, pd = frames(48, 80)
    args = args_of(img, pd, *A)
    step(eng, off, args, ((0, 3), (0, 3)))
    assert eng.last_frame_cache() == (0, 3, 0)
    step(eng, off, args, ((2, 1), (2, 1)))
    assert eng.last_frame_cache() == (2, 1, 0)
    step(eng, off, args, ((2, 1), (2, 1)))


def test_a_side_outside_the_admission_bound_neither_reads_nor_writes(eng, off):
    img, pd = frames(64, 96)
    assert not fits(5, 4, 24) and fits(5, 2, 24)
    args = args_of(img, pd, [0, 1, 2, 3, 0], [4, 5, 4, 5, 5])
    step(eng, off, args, ((0, 0), (0, 2)), sides=(4, 2, False, True))
    step(eng, off, args, ((0, 0), (2, 0)), sides=(4, 2, False, True))
    # side 1 wrote nothing of 0 and 1: when it merges with them they are misses, though the frame cache holds them
    step(eng, off, args_of(img, pd, [0, 0, 1, 1, 0], [4, 5, 4, 5, 5]), ((0, 2), (2, 0)), sides=(2, 2, True, True))
    assert eng.last_frame_cache() == (4, 0, 0)


def test_bypasses(eng, off):
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    step(eng, off, args, ((0, 3), (0, 3)))
    for e in (eng, off):
        e.set_dedup_head(False)
    step(eng, off, args, NONE, sides=(5, 5, False, False))
    for e in (eng, off):
        e.set_dedup_head(True)
    step(eng, off, args, ((3, 0), (3, 0)))                  # the stored frames are still there
    for e in (eng, off):
        e.set_tap_level(3)
    step(eng, off, args, NONE)
    for e in (eng, off):
        e.set_tap_level(0)
    step(eng, off, args, ((3, 0), (3, 0)))
    for e in (eng, off):
        e.set_dedup(0)
    step(eng, off, args, NONE)
    for e in (eng, off):
        e.set_dedup(1)                                      # (a change of the dedup mode drops the entries)
    step(eng, off, args, ((0, 3), (0, 3)))
    step(eng, off, args, ((3, 0), (3, 0)))
    # decode does not use it
    f = eng.encode(torch.stack([img[i] for i in (0, 1, 2)]))
    st = lambda items, idx: torch.stack([items[i] for i in idx]).contiguous()
    dec = eng.decode(st(f, A[0]), st(f, A[1]), args[2], args[3], 64, 96)
    assert eng.last_head_products() == NONE and eng.last_dedup_sides() == (3, 3, True, True)
    same(dec, run(off, args))


def test_everything_that_drops_the_frame_cache_drops_it(eng, off):
    from align3r_amd._lib import check, ptr, stream_ptr
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    hit, miss = ((3, 0), (3, 0)), ((0, 3), (0, 3))
    step(eng, off, args, miss)
    step(eng, off, args, hit)
    # one weight of a head set again (the same values) and the handle finalized again
    name = "downstream_head1.dpt.scratch.refinenet1.resConfUnit1.conv2.bias"
    for e in (eng, off):
        t = e.weights[name]
        check(e.lib.a3r_model_set_weight(e.handle, name.encode(), ptr(t), t.dim(), (C.c_int64 * t.dim())(*t.shape)), name)
        check(e.lib.a3r_model_finalize(e.handle, ptr(e.packed), e.packed.numel(), stream_ptr()), "a3r_model_finalize")
    step(eng, off, args, miss)
    step(eng, off, args, hit)
    for e in (eng, off):
        e.reset_ranges()
    step(eng, off, args, miss)
    step(eng, off, args, hit)
    for e in (eng, off):
        e.set_dedup(2)
    step(eng, off, args, NONE, sides=(5, 5, False, False))  # (the constant key collides: the plain head)
    for e in (eng, off):
        e.set_dedup(1)
    step(eng, off, args, miss)
    step(eng, off, args, hit)
    # another resolution, and back
    img2, pd2 = frames(48, 80)
    step(eng, off, args_of(img2, pd2, *A), miss)
    step(eng, off, args, miss)
    step(eng, off, args, hit)
    # a failed call: a workspace one byte short
    ws = eng.workspace
    out = {k: torch.empty_like(v) for k, v in run(off, args).items()}
    rc = eng.lib.a3r_model_forward(eng.handle, ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]), 5, 64, 96, ptr(out["pts3d_1"]),
                                   ptr(out["conf_1"]), ptr(out["pts3d_2"]), ptr(out["conf_2"]), ptr(ws), eng.workspace_bytes(5, 64, 96) - 1,
                                   stream_ptr())
    assert rc != 0
    same(run(eng, args), run(off, args))
    assert eng.last_head_products() == hit                  # (refused before the lookup: nothing was touched)
    # a call that fails after the handle has begun: img1 four bytes off a 16-byte boundary is refused by the duplicate search
    # before anything is launched, and the handle drops what it has stored -- the head bits with the frame cache's table
    shifted = torch.empty(args[0].numel() + 1, device="cuda")[1:].view_as(args[0])
    shifted.copy_(args[0])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for e in (eng, off):
        rc = e.lib.a3r_model_forward(e.handle, ptr(shifted), ptr(args[1]), ptr(args[2]), ptr(args[3]), 5, 64, 96, ptr(out["pts3d_1"]),
                                     ptr(out["conf_1"]), ptr(out["pts3d_2"]), ptr(out["conf_2"]), ptr(e.workspace), e.workspace.numel(),
                                     stream_ptr())
        assert rc != 0
    step(eng, off, args, miss)
    assert eng.last_frame_cache() == (0, 3, 0)
    step(eng, off, args, hit)
    # a storage set again forgets
    eng.set_head_products(int(eng.lib.a3r_model_head_products_bytes(eng.handle, 64, 96, eng.frame_cache)))
    step(eng, off, args, miss)
    step(eng, off, args, hit)


def test_the_switches_and_a_smaller_storage(monkeypatch):
    from align3r_amd._lib import check, ptr
    img, pd = frames(48, 80)
    args = args_of(img, pd, *A)
    off = _engine(8, head_products=False)
    monkeypatch.setenv("A3R_HEAD_PRODUCTS", "0")
    e = _engine(8)
    assert not e.head_products
    step(e, off, args, NONE)
    step(e, off, args, NONE)
    assert e._hp_store is None
    monkeypatch.delenv("A3R_HEAD_PRODUCTS")
    # a storage one byte short of the frame cache's entry count is ignored and never written; with as many it is used and
    # nothing is written behind it
    e = _engine(3, head_products=False)
    off3 = _engine(3, head_products=False)
    step(e, off3, args, NONE)
    n, guard = int(e.lib.a3r_model_head_products_bytes(e.handle, 48, 80, 3)), 4096
    assert n == 3 * (2 * 4096 + 4 * 16 * 15 * TINY.feature_dim * 4)
    assert int(e.lib.a3r_model_head_products_bytes(e.handle, 48, 81, 3)) == 0
    store = torch.full((n + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    check(e.lib.a3r_model_set_head_products(e.handle, ptr(store), n - 1), "a3r_model_set_head_products")
    step(e, off3, args, NONE)
    torch.cuda.synchronize()
    assert bool((store == 0x5A).all())
    check(e.lib.a3r_model_set_head_products(e.handle, ptr(store), n), "a3r_model_set_head_products")
    step(e, off3, args, ((0, 3), (0, 3)))
    step(e, off3, args, ((3, 0), (3, 0)))
    step(e, off3, args_of(img, pd, [3, 4, 5, 3, 4], [4, 5, 3, 5, 3]), ((0, 3), (0, 3)))
    torch.cuda.synchronize()
    assert bool((store[n:] == 0x5A).all()) and not bool((store[:n] == 0x5A).all())


def test_range_control_repeats_equally():
    """the scaled weights of tests/test_gpu_dedup_head.py::test_range_control_repeats_equally: the level-0 sites leave their band
    on the first attempt; with the storage on and off the engines repeat equally often and end with the same scales and outputs,
    and the repeated forward found nothing (the adjustment dropped what the first attempt stored)"""
    sd = {k: np.array(v, copy=True) for k, v in synthetic_state_dict(TINY, 0).items()}
    heads = ("downstream_head1.dpt.", "downstream_head2.dpt.")
    for k in ("enc_norm.weight", "enc_norm.bias"):
        sd[k] = (sd[k] * np.float32(2.0 ** -20)).astype(np.float32)
    for k in ["decoder_embed.weight"] + [h + "act_postprocess.0.0.weight" for h in heads]:
        sd[k] = (sd[k] * np.float32(2.0 ** 20)).astype(np.float32)
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    res = {}
    for on in (False, True):
        e = _engine(8, sd, head_products=on)
        e.reset_ranges()
        out = run(e, args)
        res[on] = (e.range_reruns, e.site_scales(0).copy(), out, e.last_dedup_sides(), e.last_head_products())
        again = run(e, args)
        same(again, out)
        assert e.range_reruns == res[on][0]
        assert e.last_head_products() == (((3, 0), (3, 0)) if on else NONE)
    assert res[False][0] >= 1 and res[True][0] == res[False][0]
    assert res[True][3] == (3, 3, True, True) and res[True][4] == ((0, 3), (0, 3))
    assert np.array_equal(res[False][1], res[True][1])
    same(res[True][2], res[False][2])


# ---- the two source-indexed combine entry points alone
def _sources(kind, S, g):
    """per slot: an entry of the storage (>= 0) or ~(fresh block)"""
    if kind == "stored":
        return [int(x) for x in torch.randint(0, 4, (S,), generator=g)]
    if kind == "fresh":
        return [~int(x) for x in torch.randint(0, 2, (S,), generator=g)]
    return [2, ~1, 0][:S] if S <= 3 else [2, ~1, 0] + [~0] * (S - 3)


@pytest.mark.parametrize("kind", ["stored", "fresh", "mixed"])
@pytest.mark.parametrize("P,Cc", [(5, 8), (24, 16), (24, 8), (5, 16)])
def test_combine_resid_src(kind, P, Cc):
    from align3r_amd import _lib, ops
    S, scale = 3, 2.0
    g = torch.Generator().manual_seed(P * 100 + Cc)
    dg = torch.Generator(device="cuda").manual_seed(P * 100 + Cc)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=dg) * 3
    # the storage: 4 entries of [2 sides][r0, c][P Cc] floats; the side under test is side 1
    store = rnd(4, 2, 2, P, Cc)
    fc, fr, p2 = rnd(2, P, Cc), rnd(2, P, Cc), rnd(S, P, Cc)
    src = _sources(kind, S, g)
    want = torch.stack([(store[e, 1, 1] + (store[e, 1, 0] + p2[b])) if e >= 0 else (fc[~e] + (fr[~e] + p2[b])) for b, e in enumerate(src)])
    m = torch.tensor(src, dtype=torch.int32, device="cuda")
    s = torch.full((S, P, Cc), float("nan"), device="cuda")
    sr2 = torch.zeros(S * P * Cc * 4, dtype=torch.uint8, device="cuda")
    word = ops.absmax_word("cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    fresh_c, fresh_r = (None, None) if kind == "stored" else (fc, fr)
    sc, sr = (None, None) if kind == "fresh" else (store[0, 1, 1], store[0, 1, 0])
    rc = _lib.load().a3r_combine_resid_fh2_src(p(fresh_c), p(fresh_r), p(sc), p(sr), 4 * P * Cc, p(m), p(p2), p(s), p(sr2), S, P, Cc, scale,
                                               p(word), _lib.stream_ptr())
    assert rc == 0
    assert torch.equal(s, want)
    w2 = ops.absmax_word("cuda")
    split = ops.split_fh2(torch.relu(want), scale, w2)
    assert torch.equal(sr2, split.data)
    assert int(word.item()) == int(w2.item())


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("kind", ["stored", "fresh", "mixed"])
@pytest.mark.parametrize("H,W,Hc,Wc,Cc", [(1, 5, 1, 5, 8), (4, 6, 8, 3, 16), (3, 5, 5, 1, 8), (3, 8, 4, 6, 16)])
def test_upsample2x_combine_src(form, kind, H, W, Hc, Wc, Cc):
    """P = Hc Wc = 5 and 24, a crop smaller than 2 H x 2 W; both kernel forms"""
    from align3r_amd import _lib, ops
    lib = _lib.load()
    S, scale, P = 3, 0.5, Hc * Wc
    assert P in (5, 24) and Hc <= 2 * H and Wc <= 2 * W and (Hc < 2 * H or Wc < 2 * W)
    g = torch.Generator().manual_seed(P * 100 + Cc + H)
    dg = torch.Generator(device="cuda").manual_seed(P * 100 + Cc + H)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=dg) * 3
    store = rnd(4, 2, 2, Hc, Wc, Cc)
    fc, fr, x = rnd(2, Hc, Wc, Cc), rnd(2, Hc, Wc, Cc), rnd(S, H, W, Cc)
    src = _sources(kind, S, g)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    prev = lib.a3r_upsample2x_set_form(form)
    try:
        p2 = torch.empty(S, Hc, Wc, Cc, device="cuda")
        assert lib.a3r_upsample2x(p(x), p(p2), S, H, W, Cc, Hc, Wc, _lib.stream_ptr()) == 0
        m = torch.tensor(src, dtype=torch.int32, device="cuda")
        s = torch.full((S, Hc, Wc, Cc), float("nan"), device="cuda")
        sr2 = torch.zeros(S * P * Cc * 4, dtype=torch.uint8, device="cuda")
        word = ops.absmax_word("cuda")
        fresh_c, fresh_r = (None, None) if kind == "stored" else (fc, fr)
        sc, sr = (None, None) if kind == "fresh" else (store[0, 0, 1], store[0, 0, 0])
        rc = lib.a3r_upsample2x_combine_fh2_src(p(x), p(fresh_c), p(fresh_r), p(sc), p(sr), 4 * P * Cc, p(m), p(s), p(sr2), S, H, W, Cc, Hc,
                                                Wc, scale, p(word), _lib.stream_ptr())
        assert rc == 0
    finally:
        lib.a3r_upsample2x_set_form(prev)
    want = torch.stack([(store[e, 0, 1] + (store[e, 0, 0] + p2[b])) if e >= 0 else (fc[~e] + (fr[~e] + p2[b])) for b, e in enumerate(src)])
    assert torch.equal(s, want)
    w2 = ops.absmax_word("cuda")
    split = ops.split_fh2(torch.relu(want), scale, w2)
    assert torch.equal(sr2, split.data)
    assert int(word.item()) == int(w2.item())
