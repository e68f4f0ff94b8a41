"""GPU: the frame products a handle keeps across forward calls (include/a3r.h, a3r_model_set_frame_products): the depth-prior token
branch -- patch_embed_point_cloud, dec_blocks_pc, the zero-convs -- runs only on the pred_depth maps the storage does not hold, and
the decoder's gather-add passes read the stored rows in place.  What is pinned here is that nothing else changes: every output
equals, bit for bit, that of a handle without any storage, whatever mixture of stored and new maps a call holds; the report counts
them; a map that differs from a stored one in a single bit (or under a constant key) is never taken for it; the least recently
used entry makes room; statistics and scales of a repeated batch are the plain handle's; weights, scales and resolution drop the
entries; the switches bypass it; a storage with fewer entries than the frame cache is ignored and nothing is written behind either.
TINY config, synthetic weights, 64x96 and 48x80 (N = 24 and 15), B = 3..4; 256x256 where block 0 must run on entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_view_arrays
from align3r_amd.weights import TINY, synthetic_state_dict

pytestmark = pytest.mark.gpu
KEYS = ("pts3d_1", "conf_1", "pts3d_2", "conf_2")


def _engine(frame_cache, sd=None, **kw):
    from align3r_amd.engine import PairEngine
    return PairEngine(TINY, sd if sd is not None else synthetic_state_dict(TINY, 0), frame_cache=frame_cache, **kw)


@pytest.fixture()
def plain():
    """the handle without any storage that every output is compared with (a new one per test, as the handle under test is: both
    then see the same calls and settle on the same scales)"""
    e = _engine(0)
    assert e.frame_cache == 0 and e._fp_store is None
    return e


@pytest.fixture()
def eng():
    e = _engine(8)
    assert e.frame_products
    return e


_frames = {}


def frames(H, W):
    if (H, W) not in _frames:
        v = make_view_arrays(7, H, W, seed=5)
        _frames[H, W] = ([torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v])
    return _frames[H, W]


def args_of(img, pd, i1, i2, d1=None, d2=None):
    st = lambda items, idx: torch.stack([items[i] for i in idx]).contiguous()
    return st(img, i1), st(img, i2), st(pd, i1 if d1 is None else d1), st(pd, i2 if d2 is None else d2)


def run(e, args):
    return {k: t.clone() for k, t in e.forward(*args).items()}


def same(out, ref):
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k


A = ([0, 1, 2, 0], [1, 2, 0, 2])          # frames 0 1 2, B = 4
B_ = ([2, 3, 4], [3, 4, 2])               # frames 2 3 4, B = 3: 2 is old after A


@pytest.mark.parametrize("hw", [(64, 96), (48, 80)])
def test_same_batch_twice(eng, plain, hw):
    img, pd = frames(*hw)
    args = args_of(img, pd, *A)
    ref = run(plain, args)
    want = (plain.last_dedup(), plain.last_dedup_sides(), plain.last_dedup_entries())
    ref_stats, ref_scales = plain.site_stats(), plain.site_scales(0)
    assert plain.last_frame_products() == (0, 0, 0)
    first = run(eng, args)
    assert eng.last_frame_products() == (0, 3, 0) and eng.last_frame_cache() == (0, 3, 0)
    st1 = eng.site_stats()
    second = run(eng, args)
    assert eng.last_frame_products() == (3, 0, 0) and eng.last_frame_cache() == (3, 0, 0)
    same(first, ref)
    same(second, ref)
    st2 = eng.site_stats()
    assert st1.tobytes() == ref_stats.tobytes() and st2.tobytes() == ref_stats.tobytes()
    assert eng.site_scales(0).tobytes() == ref_scales.tobytes()
    assert (eng.last_dedup(), eng.last_dedup_sides(), eng.last_dedup_entries()) == want
    assert eng.range_reruns == plain.range_reruns


def test_overlapping_batches(eng, plain):
    img, pd = frames(64, 96)
    same(run(eng, args_of(img, pd, *A)), run(plain, args_of(img, pd, *A)))
    same(run(eng, args_of(img, pd, *B_)), run(plain, args_of(img, pd, *B_)))
    assert eng.last_frame_products() == (1, 2, 0)
    # every prior slot distinct (nothing to merge inside the call), half of them stored: 0 and 3 against 5 and 6
    c = ([0, 5], [6, 3])
    same(run(eng, args_of(img, pd, *c)), run(plain, args_of(img, pd, *c)))
    assert eng.last_dedup()[1] == 4 and eng.last_frame_products() == (2, 2, 0)
    # and all of them stored
    same(run(eng, args_of(img, pd, *c)), run(plain, args_of(img, pd, *c)))
    assert eng.last_dedup()[1] == 4 and eng.last_frame_products() == (4, 0, 0)


def test_images_and_priors_are_looked_up_apart(eng, plain):
    img, pd = frames(64, 96)
    same(run(eng, args_of(img, pd, *A)), run(plain, args_of(img, pd, *A)))
    # the same images with other priors: prior misses, image hits
    d = args_of(img, pd, *A, d1=[3, 4, 5, 3], d2=[4, 5, 3, 5])
    same(run(eng, d), run(plain, d))
    assert eng.last_frame_cache() == (3, 0, 0) and eng.last_frame_products() == (0, 3, 0)
    # the first priors with other images: the converse
    d = args_of(img, pd, [4, 5, 6, 4], [5, 6, 4, 6], d1=A[0], d2=A[1])
    same(run(eng, d), run(plain, d))
    assert eng.last_frame_cache() == (0, 3, 0) and eng.last_frame_products() == (3, 0, 0)
    # an image with two priors and a prior with two images, half of the priors stored
    d = args_of(img, pd, [0, 0, 1], [1, 1, 0], d1=[0, 6, 6], d2=[6, 0, 1])
    same(run(eng, d), run(plain, d))
    assert eng.last_frame_products() == (2, 1, 0)


@pytest.mark.parametrize("case", ["one_ulp", "negative_zero"])
def test_one_bit_changed_misses(eng, plain, case):
    img, pd = frames(48, 80)
    a = pd[0].clone()
    b = a.clone()
    if case == "one_ulp":
        b.view(torch.int32).view(-1)[-1] ^= 1
    else:
        a.view(-1)[777] = 0.0
        b.view(-1)[777] = -0.0
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    im = args_of(img, pd, [0, 1, 0], [1, 0, 2])[:2]
    first = (*im, torch.stack([a, pd[1], a]), torch.stack([pd[1], a, pd[2]]))
    then = (*im, torch.stack([b, pd[1], b]), torch.stack([pd[1], b, pd[2]]))
    same(run(eng, first), run(plain, first))
    assert eng.last_frame_products() == (0, 3, 0)
    same(run(eng, then), run(plain, then))
    assert eng.last_frame_products() == (2, 1, 0)                 # b is not a
    same(run(eng, first), run(plain, first))
    assert eng.last_frame_products() == (3, 0, 0)                 # and both are kept


def test_constant_key(eng, plain):
    """mode 2: every key is zero, so the comparison alone tells the stored maps apart"""
    img, pd = frames(64, 96)
    eng.set_dedup(2)
    try:
        for n, (f, want) in enumerate([(0, (0, 1, 0)), (1, (0, 1, 0)), (0, (1, 0, 0)), (1, (1, 0, 0)), (2, (0, 1, 0))]):
            args = args_of(img, pd, [f] * 3, [f] * 3)
            same(run(eng, args), run(plain, args))
            assert eng.last_dedup() == (1, 1, False) and eng.last_frame_products() == want, (n, eng.last_frame_products())
    finally:
        eng.set_dedup(1)


def table_model(cap, calls):
    """what FrameCacheTable does (csrc/dedup.h, checked against a naive model by test_frame_cache_cpu.py): (hits, misses,
    evictions) of each call, a call being the list of its distinct items in slot order"""
    held, order, out = {}, [], []              # item -> entry; entries from least to most recently used
    for fr in calls:
        used = {held[f] for f in fr if f in held}
        ent, n = [], [0, 0, 0]
        for f in fr:
            if f in held:
                n[0] += 1
                ent.append(held[f])
                continue
            n[1] += 1
            free = [e for e in range(cap) if e not in held.values() and e not in used]
            lru = [e for e in order if e not in used]
            e = free[0] if free else lru[0] if lru else None
            if e is not None:
                if not free:
                    n[2] += 1
                    held = {g: x for g, x in held.items() if x != e}
                used.add(e)
                held[f] = e
            ent.append(e)
        for e in ent:
            if e is not None:
                order = [x for x in order if x != e] + [e]
        out.append(tuple(n))
    return out


def distinct_in_slot_order(i1, i2):
    seen = []
    for f in list(i1) + list(i2):
        if f not in seen:
            seen.append(f)
    return seen


def test_eviction_and_more_misses_than_entries(plain):
    """the priors follow an order of their own (d1 / d2), so that their table's victims are not the frame cache's"""
    img, pd = frames(48, 80)
    eng = _engine(0)
    eng.set_frame_cache(2, 48, 80)
    assert eng._fp_store is not None
    im = ([0, 1, 0, 1], [1, 0, 1, 0])
    calls = [([0, 1, 0], [1, 0, 1]), ([1, 2, 1], [2, 1, 2]), ([0, 2, 0], [2, 0, 2]), ([3, 4, 5, 6], [4, 5, 6, 3]), ([3, 0, 3], [0, 3, 0]),
             ([3, 1, 2, 5], [1, 2, 5, 3]), ([2, 3, 4], [3, 4, 2]), ([4, 2, 4], [2, 4, 2])]
    want = table_model(2, [distinct_in_slot_order(*c) for c in calls])
    # the cases this test is about: one victim, more new maps than entries, and the same beside a map that is read
    assert want[1] == (1, 1, 1) and want[3] == (0, 4, 2) and want[5] == (1, 3, 1), want
    for c, w in zip(calls, want):
        n = len(c[0])
        args = args_of(img, pd, im[0][:n], im[1][:n], d1=c[0], d2=c[1])
        same(run(eng, args), run(plain, args))
        assert eng.last_frame_products() == w, (c, eng.last_frame_products(), w)


def test_flushes(plain):
    img, pd = frames(64, 96)
    sd = synthetic_state_dict(TINY, 0)
    eng = _engine(8, sd)
    args = args_of(img, pd, *A)
    ref = run(plain, args)
    same(run(eng, args), ref)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (3, 0, 0)
    # one weight of the prior branch set again (the same values): the handle is finalized again and has forgotten its maps
    from align3r_amd._lib import check, ptr, stream_ptr
    name = "dec_blocks_pc.0.mlp.fc1.bias"
    t = eng.weights[name]
    check(eng.lib.a3r_model_set_weight(eng.handle, name.encode(), ptr(t), t.dim(), (C.c_int64 * t.dim())(*t.shape)), name)
    check(eng.lib.a3r_model_finalize(eng.handle, ptr(eng.packed), eng.packed.numel(), stream_ptr()), "a3r_model_finalize")
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)
    # another resolution, and back
    img2, pd2 = frames(48, 80)
    small = args_of(img2, pd2, *A)
    same(run(eng, small), run(plain, small))
    assert eng.last_frame_products() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (3, 0, 0)
    eng.reset_ranges()
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)


def test_flush_after_a_range_adjustment():
    """weights that push a site of the prior branch out of its band (patch_embed_point_cloud's output ~1e-6 of its usual size, the
    first zero-conv scaled back): the first forward stores its maps, the range check moves a site and the repeated forward must
    run the branch again, with the new scales"""
    sd = {k: np.array(v, copy=True) for k, v in synthetic_state_dict(TINY, 0).items()}
    for k in ("patch_embed_point_cloud.proj.weight", "patch_embed_point_cloud.proj.bias"):
        sd[k] = (sd[k] * np.float32(2.0 ** -20)).astype(np.float32)
    sd["zero_convs.0.0.weight"] = (sd["zero_convs.0.0.weight"] * np.float32(2.0 ** 20)).astype(np.float32)
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    off, eng = _engine(0, sd), _engine(8, sd)
    ref = run(off, args)
    assert off.range_reruns >= 1
    out = run(eng, args)
    assert eng.range_reruns == off.range_reruns
    assert eng.last_frame_products() == (0, 3, 0)          # the repeated forward found nothing
    same(out, ref)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (3, 0, 0) and eng.range_reruns == off.range_reruns
    assert eng.site_scales(0).tobytes() == off.site_scales(0).tobytes()


def test_bypasses(eng, plain):
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    ref = run(plain, args)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)
    eng.set_tap_level(3)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 0, 0)
    eng.set_tap_level(0)
    eng.set_dedup(0)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 0, 0)
    eng.set_dedup(1)                                      # (a change of the dedup mode drops the entries)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)
    # the decoder's and the heads' switches do not concern the stored maps: a handle with the decoder's switch off reads the same
    # stored rows and statistics words as one with it on (tests/test_gpu_dedup_decoder.py compares the two over overlapping calls)
    want_stats = eng.site_stats()
    for switch in (eng.set_dedup_decoder, eng.set_dedup_head):
        switch(0)
        same(run(eng, args), ref)
        assert eng.last_frame_products() == (3, 0, 0) and eng.last_frame_cache() == (3, 0, 0)
        assert eng.site_stats().tobytes() == want_stats.tobytes()
        switch(1)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (3, 0, 0)


def test_the_environment_switches_it_off(monkeypatch, plain):
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    monkeypatch.setenv("A3R_FRAME_PRODUCTS", "0")
    eng = _engine(8)
    assert not eng.frame_products
    ref = run(plain, args)
    same(run(eng, args), ref)
    same(run(eng, args), ref)
    assert eng._fp_store is None and eng.last_frame_products() == (0, 0, 0) and eng.last_frame_cache() == (3, 0, 0)
    monkeypatch.delenv("A3R_FRAME_PRODUCTS")
    assert not _engine(8, frame_products=False).frame_products


def test_a_storage_with_fewer_entries_than_the_frame_cache_is_ignored(plain):
    img, pd = frames(48, 80)
    args = args_of(img, pd, *A)
    eng = _engine(0, frame_products=False)
    from align3r_amd._lib import check, ptr
    frames_kept, guard = 3, 4096
    nc = int(eng.lib.a3r_model_frame_cache_bytes(eng.handle, 48, 80, frames_kept))
    npr = int(eng.lib.a3r_model_frame_products_bytes(eng.handle, 48, 80, frames_kept))
    assert npr > 0 and npr == frames_kept * int(eng.lib.a3r_model_frame_products_bytes(eng.handle, 48, 80, 1))
    assert int(eng.lib.a3r_model_frame_products_bytes(eng.handle, 48, 81, 1)) == 0
    cache = torch.full((nc + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    prod = torch.full((npr + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    check(eng.lib.a3r_model_set_frame_cache(eng.handle, ptr(cache), nc), "a3r_model_set_frame_cache")
    # one byte short of the frame cache's entry count: the run is that of the frame cache alone, and nothing is written to it
    check(eng.lib.a3r_model_set_frame_products(eng.handle, ptr(prod), npr - 1), "a3r_model_set_frame_products")
    ref = run(plain, args)
    same(run(eng, args), ref)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (3, 0, 0) and eng.last_frame_products() == (0, 0, 0)
    torch.cuda.synchronize()
    assert bool((prod == 0x5A).all())
    # exactly as many: used, and both stay inside
    check(eng.lib.a3r_model_set_frame_products(eng.handle, ptr(prod), npr), "a3r_model_set_frame_products")
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_products() == (3, 0, 0)
    big = args_of(img, pd, [3, 4, 5, 6], [4, 5, 6, 3])    # more new maps than entries
    same(run(eng, big), run(plain, big))
    assert eng.last_frame_products() == (0, 4, 3)
    torch.cuda.synchronize()
    assert bool((prod[npr:] == 0x5A).all()) and bool((cache[nc:] == 0x5A).all())
    assert not bool((prod[:npr] == 0x5A).all())


_frames256 = []


def test_block_0_on_entries_reads_the_store(eng, plain):
    """256x256 (N = 256: whole row tiles): block 0 runs on each side's distinct (image, prior) entries, whose level-0 rows the
    gather-add pass makes from stored and fresh z_0 rows"""
    if not _frames256:
        v = make_view_arrays(5, 256, 256, 7)
        _frames256.append(([torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]))
    img, pd = _frames256[0]
    a = args_of(img, pd, [0, 1, 2, 0, 1], [1, 2, 3, 1, 2])
    ref = run(plain, a)
    assert plain.last_dedup_entries() == (3, 3, True)
    same(run(eng, a), ref)
    assert eng.last_dedup_entries() == (3, 3, True) and eng.last_frame_products() == (0, 4, 0)
    same(run(eng, a), ref)
    assert eng.last_frame_products() == (4, 0, 0)
    assert eng.site_stats().tobytes() == plain.site_stats().tobytes()
    b = args_of(img, pd, [0, 0, 1, 4, 1], [1, 4, 0, 0, 4])        # priors 0 and 1 stored, 4 new
    same(run(eng, b), run(plain, b))
    assert eng.last_dedup_entries()[2] and eng.last_frame_products() == (2, 1, 0)


# ---- the kernels alone
def p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("S,N,Cc,with_b", [(5, 15, 64, True), (5, 15, 64, False), (3, 24, 8, True),
                                           (4, 22000, 768, False)])      # 16.9 M float4: more than the capped grid holds threads
def test_gather_add_rows_src_equals_gather_add_rows(S, N, Cc, with_b):
    """rows taken from entries of a store (a stride apart, other fields between them) and from fresh blocks, against
    a3r_gather_add_rows on the same rows copied into one array"""
    from align3r_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(S * 1000 + N)
    levels = 3 if N < 1000 else 1
    cap, n_fresh, stride = 4, 2, N * Cc * levels + 8
    store = torch.randn(cap * stride, device="cuda", generator=g)
    fresh = torch.randn(n_fresh, N, Cc, device="cuda", generator=g)
    off = N * Cc if levels > 1 else 0                     # the level the pass reads: the second of three in every entry
    src = [2, ~1, 0, ~0, 3][:S]
    rows = torch.stack([store[e * stride + off:e * stride + off + N * Cc].view(N, Cc) if e >= 0 else fresh[~e] for e in src]).contiguous()
    b = torch.randn(3, N, Cc, device="cuda", generator=g)
    mb = torch.tensor([1, 0, 2, 2, 0][:S], dtype=torch.int32, device="cuda")
    x0 = torch.randn(S, N, Cc, device="cuda", generator=g)
    want, got = x0.clone(), x0.clone()
    ident = torch.arange(S, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()
    assert lib.a3r_gather_add_rows(p(rows), p(ident), p(b) if with_b else None, p(mb) if with_b else None, p(want), S, N, Cc, st) == 0
    srct = torch.tensor(src, dtype=torch.int32, device="cuda")
    assert lib.a3r_gather_add_rows_src(p(store[off:]), stride, p(fresh), p(srct), p(b) if with_b else None, p(mb) if with_b else None,
                                       p(got), S, N, Cc, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_statistics_pass_on_a_site_list_with_gaps():
    """the words of the listed sites: kept with every entry the call filled, then raised to the largest word of the entries it read
    (bit patterns of non-negative floats); every other word, and every entry the call did not touch, stays as it was"""
    from align3r_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    words_item, words_rows, cap, W = 64, 128, 5, 1024
    entry = 16 + W * 4 + 4 * 512 * 2 + (words_item + words_rows) * 4          # csrc/dedup.h, frame_cache_entry_bytes
    host = rng.integers(0, 256, cap * entry, dtype=np.uint8)
    est = np.abs(rng.standard_normal((cap, W))).astype(np.float32)
    host[cap * 16:cap * 16 + cap * W * 4] = est.view(np.uint8).reshape(-1)      # the entries' words follow the cap keys
    store = torch.from_numpy(host.copy()).cuda()
    sites = [i for lo, hi in ((0, 1), (5, 9), (31, 33), (100, 101), (700, 1024)) for i in range(lo, hi)]
    mask = np.zeros(32, np.uint32)
    for i in sites:
        mask[i // 32] |= np.uint32(1 << (i % 32))
    own = np.abs(rng.standard_normal(W)).astype(np.float32)
    own[6] = 0.0
    ent = np.array([3, -1, 0, 4], np.int32)               # filled, a miss without an entry, read, read
    miss = np.array([0, 1, -1, -1], np.int32)
    stats, ent_d, miss_d = torch.from_numpy(own.copy()).cuda(), torch.from_numpy(ent).cuda(), torch.from_numpy(miss).cuda()
    rc = lib.a3r_frame_cache_stats_sites(p(store), cap * entry, words_item, words_rows, p(ent_d), p(miss_d), 4, p(stats),
                                         mask.ctypes.data_as(C.c_void_p), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    want, want_est = own.copy(), est.copy()
    want[sites] = np.maximum(own[sites], np.maximum(est[0, sites], est[4, sites]))
    want_est[3, sites] = own[sites]
    assert stats.cpu().numpy().tobytes() == want.tobytes()
    got = store.cpu().numpy()
    assert got[cap * 16:cap * 16 + cap * W * 4].tobytes() == want_est.tobytes()
    rest = np.ones(host.size, bool)
    rest[cap * 16:cap * 16 + cap * W * 4] = False
    assert np.array_equal(got[rest], host[rest])
