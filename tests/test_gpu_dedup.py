"""GPU: a3r_model_forward / a3r_model_decode run the frame-only parts of the plan (encoder, depth-prior token branch) once per
DISTINCT image / pred_depth map of the batch (include/a3r.h, a3r_model_set_dedup).  What is pinned here: with duplicates merged
(mode 1) every output equals the plain plan's (mode 0) bit for bit, the reported counts are the true numbers of distinct inputs,
inputs that differ in a single bit are never merged, a key collision (mode 2: constant key) ends in the plain plan, the fh2 range
control sees the same sites and scales, and the workspace requirement holds.  TINY config, synthetic weights."""
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


def frames(n, H, W, seed=3):
    v = make_view_arrays(n, H, W, seed)
    return [torch.from_numpy(a[0][0]).cuda() for a in v], [torch.from_numpy(a[1][0]).cuda() for a in v]


def batch(items, idx):
    return torch.stack([items[i] for i in idx]).contiguous()


def both_modes(eng, args, want, debug_key=False):
    """mode 0 against mode 1 (or 2): equal bits on all four outputs; `want` = (distinct images, distinct maps, fell_back)."""
    eng.set_dedup(0)
    ref = {k: t.clone() for k, t in eng.forward(*args).items()}
    assert eng.last_dedup() == (2 * len(args[0]), 2 * len(args[0]), False)
    eng.set_dedup(2 if debug_key else 1)
    try:
        out = eng.forward(*args)
        assert eng.last_dedup() == want, eng.last_dedup()
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), k
    finally:
        eng.set_dedup(1)
    return ref


I1, I2 = [0, 0, 1, 2, 1], [1, 2, 0, 0, 2]         # B = 5 from 3 frames, sides swapped


def test_basic_duplicates(eng):
    img, pd = frames(3, 64, 96)
    both_modes(eng, (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2)), (3, 3, False))


def test_images_and_depth_priors_are_merged_independently(eng):
    img, pd = frames(10, 64, 96)
    d1, d2 = list(range(5)), list(range(5, 10))
    both_modes(eng, (batch(img, I1), batch(img, I2), batch(pd, d1), batch(pd, d2)), (3, 10, False))
    both_modes(eng, (batch(img, d1), batch(img, d2), batch(pd, I1), batch(pd, I2)), (10, 3, False))


@pytest.mark.parametrize("case", ["lowest_bit_last_pixel", "negative_zero", "same_magnitude_elsewhere"])
def test_near_duplicates_stay_distinct(eng, case):
    img, pd = frames(2, 64, 96)
    a = img[0].clone()
    b = a.clone()
    if case == "lowest_bit_last_pixel":
        w = b.view(torch.int32).view(-1)
        w[-1] ^= 1
    elif case == "negative_zero":
        a.view(-1)[1234] = 0.0
        b.view(-1)[1234] = -0.0
    else:                              # two unequal values trade places: the same multiset of words at other positions
        f = b.view(-1)
        assert torch.isfinite(a).all() and f[100] != f[5000]
        f[100], f[5000] = a.view(-1)[5000], a.view(-1)[100]
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a and b share every batch with a true duplicate (a twice), images and maps alike: [a, b, a] x [f1, f1, b]
    pa, pb = pd[0], pd[0].clone()
    pb.view(torch.int32).view(-1)[-1] ^= 1
    img1, img2 = torch.stack([a, b, a]), torch.stack([img[1], img[1], b])
    pd1, pd2 = torch.stack([pa, pb, pa]), torch.stack([pd[1], pd[1], pb])
    both_modes(eng, (img1, img2, pd1, pd2), (3, 3, False))


def test_extremes_of_the_distinct_count(eng):
    img, pd = frames(6, 64, 96)
    a, b = [0, 1, 2], [3, 4, 5]
    both_modes(eng, (batch(img, a), batch(img, b), batch(pd, a), batch(pd, b)), (6, 6, False))              # all distinct: today's plan
    z = [0, 0, 0]
    both_modes(eng, (batch(img, z), batch(img, z), batch(pd, z), batch(pd, z)), (1, 1, False))              # all equal
    both_modes(eng, (batch(img, [2]), batch(img, [2]), batch(pd, [2]), batch(pd, [2])), (1, 1, False))      # B = 1, img1 == img2
    c = [3, 4, 0]
    both_modes(eng, (batch(img, a), batch(img, c), batch(pd, a), batch(pd, c)), (5, 5, False))              # 2 B - 1


def test_key_collisions_end_in_the_plain_plan(eng):
    """Constant key: every slot is proposed as a duplicate of slot 0; the comparison refuses, the call runs the plain plan."""
    img, pd = frames(6, 64, 96)
    both_modes(eng, (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2)), (10, 10, True), debug_key=True)
    a, b = [0, 1, 2], [3, 4, 5]
    both_modes(eng, (batch(img, a), batch(img, b), batch(pd, a), batch(pd, b)), (6, 6, True), debug_key=True)
    z = [0, 0]
    both_modes(eng, (batch(img, z), batch(img, z), batch(pd, z), batch(pd, z)), (1, 1, False), debug_key=True)   # truly all equal


@pytest.mark.parametrize("gemm", ["fh2", "bf3", "f32"])
def test_odd_row_count_of_the_distinct_frames(monkeypatch, gemm):
    """48x80: 15 tokens per frame, 3 distinct frames = 45 rows (odd) beside 2 B N = 90 or 150 rows: the row-pair layout of the bf3
    GEMM inputs applies to the 2 B N-row buffers (B N even) and cannot apply to the distinct frames' stage."""
    monkeypatch.setenv("A3R_GEMM", gemm)
    e = _engine()
    img, pd = frames(3, 48, 80)
    i1, i2 = [0, 0, 1, 2], [1, 2, 0, 0]                          # B N = 60: row pairs on
    both_modes(e, (batch(img, i1), batch(img, i2), batch(pd, i1), batch(pd, i2)), (3, 3, False))
    both_modes(e, (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2)), (3, 3, False))     # B N = 75: plain rows


def test_decode_with_duplicated_depth_priors(eng):
    img, pd = frames(3, 64, 96)
    f = eng.encode(batch(img, [0, 1, 2]))
    f1, f2, d1, d2 = batch(f, I1), batch(f, I2), batch(pd, I1), batch(pd, I2)
    eng.set_dedup(0)
    ref = {k: t.clone() for k, t in eng.decode(f1, f2, d1, d2, 64, 96).items()}
    eng.set_dedup(1)
    out = eng.decode(f1, f2, d1, d2, 64, 96)
    assert eng.last_dedup() == (10, 3, False)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
    fwd = eng.forward(batch(img, I1), batch(img, I2), d1, d2)
    for k in KEYS:
        assert torch.equal(out[k], fwd[k]), k


def test_range_control_sees_the_same_sites(eng):
    """Weights scaled so that sites leave their band on the first attempt (the encoder output ~1e-6, as in test_gpu_fh2_range):
    from reset scales, merged and plain calls repeat equally often and end with the same scales and the same outputs."""
    from align3r_amd.engine import PairEngine
    sd = {k: np.array(v, copy=True) for k, v in synthetic_state_dict(TINY, 0).items()}
    heads = ("downstream_head1.dpt.", "downstream_head2.dpt.")
    for k in ("enc_norm.weight", "enc_norm.bias"):
        sd[k] = (sd[k] * np.float32(2.0 ** -20)).astype(np.float32)
    for k in ["decoder_embed.weight"] + [h + "act_postprocess.0.0.weight" for h in heads]:
        sd[k] = (sd[k] * np.float32(2.0 ** 20)).astype(np.float32)
    e = PairEngine(TINY, sd)
    img, pd = frames(3, 64, 96)
    args = (batch(img, I1), batch(img, I2), batch(pd, I1), batch(pd, I2))
    res = {}
    for mode in (0, 1):
        e.set_dedup(mode)
        e.reset_ranges()
        n0 = e.range_reruns
        out = {k: t.clone() for k, t in e.forward(*args).items()}
        res[mode] = (e.range_reruns - n0, e.site_scales(0).copy(), out, e.last_dedup())
    assert res[0][0] >= 1 and res[1][0] == res[0][0]
    assert res[1][3] == (3, 3, False)
    assert res[0][1].shape == res[1][1].shape and np.array_equal(res[0][1], res[1][1])
    for k in KEYS:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


@pytest.mark.parametrize("case", ["duplicated", "one_duplicate"])
def test_merged_forward_stays_inside_its_buffers(eng, case):
    """As test_gpu_model.py::test_forward_stays_inside_its_buffers, for the plans on distinct inputs: a workspace of EXACTLY
    a3r_model_workspace_bytes and outputs cut from one allocation, each followed by a canary region."""
    H, W = 48, 80
    img, pd = frames(6, H, W)
    i1, i2 = (I1, I2) if case == "duplicated" else ([0, 1, 2], [3, 4, 0])
    B = len(i1)
    args = (batch(img, i1), batch(img, i2), batch(pd, i1), batch(pd, i2))
    need = eng.workspace_bytes(B, H, W)
    PAD, P = 1 << 16, H * W
    sizes = [need, B * P * 3 * 4, B * P * 4, B * P * 3 * 4, B * P * 4]
    offs, total = [], PAD
    for s in sizes:
        offs.append(total)
        total += (s + 255) // 256 * 256 + PAD
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    view = lambda o, n: arena[o:o + n]
    f32 = lambda i, *shape: view(offs[i], sizes[i]).view(torch.float32).view(*shape)
    saved = eng.workspace
    eng.set_dedup(1)
    try:
        eng.workspace = view(offs[0], need)
        out = dict(pts3d_1=f32(1, B, H, W, 3), conf_1=f32(2, B, H, W), pts3d_2=f32(3, B, H, W, 3), conf_2=f32(4, B, H, W))
        eng.forward(*args, out=out)
        torch.cuda.synchronize()
        assert eng.workspace.data_ptr() == arena.data_ptr() + offs[0]
        assert eng.last_dedup() == ((3, 3, False) if case == "duplicated" else (5, 5, False))
    finally:
        eng.workspace = saved
    used = torch.zeros(total, dtype=torch.bool, device="cuda")
    for o, s in zip(offs, sizes):
        used[o:o + s] = True
    assert bool((arena[~used] == 0xA5).all()), "the forward wrote outside its workspace / output buffers"
    eng.set_dedup(0)
    try:
        ref = eng.forward(*args)
    finally:
        eng.set_dedup(1)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k


def test_inference_without_the_cache_equals_the_cached_path(tmp_path):
    """inference() on a swin-2 graph of 5 frames: the plain per-pair path (now merging duplicates inside each batch) and
    cache_encoder=True (one encode per frame) give the same bits -- the existing guarantee, reached from both sides."""
    import align3r_amd
    from align3r_amd.weights import model_string
    align3r_amd.install_as_dust3r()
    from dust3r.image_pairs import make_pairs
    from dust3r.inference import inference
    from dust3r.model import AsymmetricCroCo3DStereo, _parse_model_string, save_checkpoint
    m = AsymmetricCroCo3DStereo(**{**_parse_model_string(model_string(TINY)), "landscape_only": False})
    path = str(tmp_path / "tiny.pth")
    save_checkpoint(path, m)
    model = AsymmetricCroCo3DStereo.from_pretrained(path).to("cuda")
    H, W = 48, 64
    views = [dict(img=torch.from_numpy(i), pred_depth=torch.from_numpy(p), true_shape=np.int32([[H, W]]), idx=n, instance=str(n))
             for n, (i, p) in enumerate(make_view_arrays(5, H, W, 7))]
    pairs = make_pairs(views, scene_graph="swin-2", symmetrize=True)
    model._engine.set_dedup(1)
    a = inference(pairs, model, "cuda", batch_size=len(pairs), verbose=False)
    assert model._engine.last_dedup() == (5, 5, False)
    b = inference(pairs, model, "cuda", batch_size=len(pairs), verbose=False, cache_encoder=True)
    for side, key in (("pred1", "pts3d"), ("pred1", "conf"), ("pred2", "pts3d_in_other_view"), ("pred2", "conf")):
        assert torch.equal(a[side][key], b[side][key]), (side, key)
