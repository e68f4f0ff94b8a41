"""GPU: the frames a handle keeps across forward calls (include/a3r.h, a3r_model_set_frame_cache).  A frame found in the storage is
not encoded again; what is pinned here is that nothing else changes: every output equals, bit for bit, that of a handle without
storage, whatever mixture of stored and new frames a call holds; the reports count them; an image that differs from a stored one
in a single bit (or under a constant key) is never taken for it; the least recently used entry makes room and a call with more
new frames than entries stores some of them; the range statistics and scales of a repeated batch are the first call's; weights,
scales and resolution drop the entries; a tap level and dedup mode 0 leave the storage alone; storage without room for one entry
is refused.  TINY config, synthetic weights, 64x96 and 48x80, B = 3..4."""
import numpy as np
import pytest
import torch

from conftest import make_view_arrays
from align3r_amd.weights import TINY, synthetic_state_dict

pytestmark = pytest.mark.gpu
KEYS = ("pts3d_1", "conf_1", "pts3d_2", "conf_2")


def _engine(frame_cache, sd=None):
    from align3r_amd.engine import PairEngine
    return PairEngine(TINY, sd if sd is not None else synthetic_state_dict(TINY, 0), frame_cache=frame_cache)


@pytest.fixture()
def plain():
    """the handle without storage that every output is compared with (a new one per test, as the handle under test is: both then
    see the same calls and settle on the same scales)"""
    e = _engine(0)
    assert e.frame_cache == 0
    return e


@pytest.fixture()
def eng():
    return _engine(8)


_frames = {}


def frames(H, W):
    if (H, W) not in _frames:
        v = make_view_arrays(7, H, W, seed=5)
        _frames[H, W] = ([torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v])
    return _frames[H, W]


def args_of(img, pd, i1, i2):
    st = lambda items, idx: torch.stack([items[i] for i in idx]).contiguous()
    return st(img, i1), st(img, i2), st(pd, i1), st(pd, i2)


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
    assert plain.last_frame_cache() == (0, 0, 0)
    first = run(eng, args)
    assert eng.last_frame_cache() == (0, 3, 0)
    st1 = eng.site_stats()
    second = run(eng, args)
    assert eng.last_frame_cache() == (3, 0, 0)
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
    assert eng.last_frame_cache() == (1, 2, 0)
    # every image slot distinct (nothing to merge inside the call), half of them stored: 0 and 3 against 5 and 6
    c = ([0, 5], [6, 3])
    same(run(eng, args_of(img, pd, *c)), run(plain, args_of(img, pd, *c)))
    assert eng.last_dedup()[0] == 4 and eng.last_frame_cache() == (2, 2, 0)
    # the same frames with other depth priors: the image alone is looked up
    d = args_of(img, pd, *A)
    d = (d[0], d[1], args_of(img, pd, *B_)[2][[0, 1, 2, 0]].contiguous(), d[3])
    same(run(eng, d), run(plain, d))
    assert eng.last_frame_cache() == (3, 0, 0)


@pytest.mark.parametrize("case", ["one_ulp", "negative_zero"])
def test_one_bit_changed_misses(eng, plain, case):
    img, pd = frames(48, 80)
    a = img[0].clone()
    b = a.clone()
    if case == "one_ulp":
        b.view(torch.int32).view(-1)[-1] ^= 1
    else:
        a.view(-1)[777] = 0.0
        b.view(-1)[777] = -0.0
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    first = (torch.stack([a, img[1], a]), torch.stack([img[1], a, img[2]]), *args_of(img, pd, [0, 1, 0], [1, 0, 2])[2:])
    then = (torch.stack([b, img[1], b]), torch.stack([img[1], b, img[2]]), *first[2:])
    same(run(eng, first), run(plain, first))
    assert eng.last_frame_cache() == (0, 3, 0)
    same(run(eng, then), run(plain, then))
    assert eng.last_frame_cache() == (2, 1, 0)                    # b is not a
    same(run(eng, first), run(plain, first))
    assert eng.last_frame_cache() == (3, 0, 0)                    # and both are kept


def test_constant_key(eng, plain):
    """mode 2: every key is zero, so the comparison alone tells the stored frames apart.  (Inside one call the constant key merges
    nothing but equal slots: a call with different images runs the plain plan and leaves the storage alone.)"""
    img, pd = frames(64, 96)
    eng.set_dedup(2)
    try:
        for n, (f, want) in enumerate([(0, (0, 1, 0)), (1, (0, 1, 0)), (0, (1, 0, 0)), (1, (1, 0, 0)), (2, (0, 1, 0))]):
            args = args_of(img, pd, [f] * 3, [f] * 3)
            same(run(eng, args), run(plain, args))
            assert eng.last_dedup() == (1, 1, False) and eng.last_frame_cache() == want, (n, eng.last_frame_cache())
        mixed = args_of(img, pd, *A)
        same(run(eng, mixed), run(plain, mixed))
        assert eng.last_dedup()[2] and eng.last_frame_cache() == (0, 0, 0)
        args = args_of(img, pd, [2] * 3, [2] * 3)
        same(run(eng, args), run(plain, args))
        assert eng.last_frame_cache() == (1, 0, 0)
    finally:
        eng.set_dedup(1)


def table_model(cap, calls):
    """what FrameCacheTable does (csrc/dedup.h, checked against a naive model by test_frame_cache_cpu.py): (hits, misses,
    evictions) of each call, a call being the list of its distinct frames in slot order"""
    held, order, out = {}, [], []              # frame -> entry; entries from least to most recently used
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
    img, pd = frames(48, 80)
    eng = _engine(0)
    eng.set_frame_cache(2, 48, 80)
    calls = [([0, 1, 0], [1, 0, 1]), ([1, 2, 1], [2, 1, 2]), ([0, 2, 0], [2, 0, 2]), ([3, 4, 5, 6], [4, 5, 6, 3]), ([3, 0, 3], [0, 3, 0]),
             ([3, 1, 2, 5], [1, 2, 5, 3]), ([2, 3, 4], [3, 4, 2]), ([4, 2, 4], [2, 4, 2])]
    want = table_model(2, [distinct_in_slot_order(*c) for c in calls])
    # the cases this test is about: one victim, more new frames than entries, and the same beside a frame that is read
    assert want[1] == (1, 1, 1) and want[3] == (0, 4, 2) and want[5] == (1, 3, 1), want
    for c, w in zip(calls, want):
        args = args_of(img, pd, *c)
        same(run(eng, args), run(plain, args))
        assert eng.last_frame_cache() == w, (c, eng.last_frame_cache(), w)


def test_flushes(plain):
    img, pd = frames(64, 96)
    sd = synthetic_state_dict(TINY, 0)
    eng = _engine(8, sd)
    args = args_of(img, pd, *A)
    ref = run(plain, args)
    same(run(eng, args), ref)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (3, 0, 0)
    # one weight set again (the same values): the handle has to be finalized again and has forgotten its frames
    from align3r_amd._lib import check, ptr, stream_ptr
    import ctypes as C
    name = "enc_blocks.0.mlp.fc1.bias"
    t = eng.weights[name]
    check(eng.lib.a3r_model_set_weight(eng.handle, name.encode(), ptr(t), t.dim(), (C.c_int64 * t.dim())(*t.shape)), name)
    check(eng.lib.a3r_model_finalize(eng.handle, ptr(eng.packed), eng.packed.numel(), stream_ptr()), "a3r_model_finalize")
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 3, 0)
    # another resolution, and back
    img2, pd2 = frames(48, 80)
    small = args_of(img2, pd2, *A)
    same(run(eng, small), run(plain, small))
    assert eng.last_frame_cache() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (3, 0, 0)
    eng.reset_ranges()
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 3, 0)


def test_flush_after_a_range_adjustment():
    """the scaled weights of test_gpu_fh2_range.py (encoder output ~1e-6): the first forward stores its frames, the range check moves
    a site and the repeated forward must encode them again, with the new scales"""
    sd = {k: np.array(v, copy=True) for k, v in synthetic_state_dict(TINY, 0).items()}
    heads = ("downstream_head1.dpt.", "downstream_head2.dpt.")
    for k in ("enc_norm.weight", "enc_norm.bias"):
        sd[k] = (sd[k] * np.float32(2.0 ** -20)).astype(np.float32)
    for k in ["decoder_embed.weight"] + [h + "act_postprocess.0.0.weight" for h in heads]:
        sd[k] = (sd[k] * np.float32(2.0 ** 20)).astype(np.float32)
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    off, eng = _engine(0, sd), _engine(8, sd)
    ref = run(off, args)
    assert off.range_reruns >= 1
    out = run(eng, args)
    assert eng.range_reruns == off.range_reruns
    assert eng.last_frame_cache() == (0, 3, 0)          # the repeated forward found nothing
    same(out, ref)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (3, 0, 0) and eng.range_reruns == off.range_reruns
    assert eng.site_scales(0).tobytes() == off.site_scales(0).tobytes()


def test_bypasses(eng, plain):
    img, pd = frames(64, 96)
    args = args_of(img, pd, *A)
    ref = run(plain, args)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 3, 0)
    eng.set_tap_level(3)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 0, 0)
    eng.set_tap_level(0)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (3, 0, 0)          # the tap call left the storage alone
    eng.set_dedup(0)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 0, 0)
    eng.set_dedup(1)


def test_storage_smaller_than_one_entry_is_refused(plain):
    img, pd = frames(48, 80)
    args = args_of(img, pd, *A)
    eng = _engine(0)
    one = int(eng.lib.a3r_model_frame_cache_bytes(eng.handle, 48, 80, 1))
    assert one > 0 and int(eng.lib.a3r_model_frame_cache_bytes(eng.handle, 48, 80, 3)) == 3 * one
    assert int(eng.lib.a3r_model_frame_cache_bytes(eng.handle, 48, 81, 1)) == 0
    with pytest.raises(RuntimeError, match="too small"):
        eng.set_frame_cache(1, 48, 80, nbytes=256)
    # one byte short of an entry at this resolution: the forward is refused before anything is written behind the storage
    guard = 4096
    eng.set_frame_cache(1, 48, 80, nbytes=one - 1 + guard)
    store = eng._fc_store
    store.fill_(0x5A)
    from align3r_amd._lib import check, ptr
    check(eng.lib.a3r_model_set_frame_cache(eng.handle, ptr(store), one - 1), "a3r_model_set_frame_cache")
    with pytest.raises(RuntimeError, match="smaller than one entry"):
        eng.forward(*args)
    torch.cuda.synchronize()
    assert bool((store == 0x5A).all())
    # exactly one entry: works, and stays inside
    check(eng.lib.a3r_model_set_frame_cache(eng.handle, ptr(store), one), "a3r_model_set_frame_cache")
    ref = run(plain, args)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (0, 3, 0)
    same(run(eng, args), ref)
    assert eng.last_frame_cache() == (1, 2, 0)
    torch.cuda.synchronize()
    assert bool((store[one:] == 0x5A).all())
