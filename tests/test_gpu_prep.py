"""GPU: the preprocessing kernels (csrc/prep.hip: a3r_prep_pointmap, a3r_prep_resize3, a3r_prep_image) against the package's own host
functions on the same inputs (pixel_to_pointcloud, crop_img, ImgNorm: DESIGN 6.7).  No tolerance: equal as numbers, NaNs in the same
places.  Every case goes through crop_img(device=...), and every C call it made is replayed on buffers the test owns, outputs and
workspace inside canary arenas.  Then the special values, the focal forms, the image side, load_images(prep_device=...) end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import prep_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 256


def device_pointmap(img, depth, focal, size, square_ok, crop):
    from align3r_amd.dust3r.utils.image_pose import crop_img
    return crop_img(img, size, (depth, focal), square_ok=square_ok, crop=crop, device="cuda")


@pytest.fixture
def calls(monkeypatch):
    """Records (name, source, focal, tables, crop, result) of every ops.prep_pointmap / ops.prep_resize3 call."""
    from align3r_amd import ops
    seen = []
    pm, rs = ops.prep_pointmap, ops.prep_resize3

    def prep_pointmap(depth, focal, tables, crop=None):
        out = pm(depth, focal, tables, crop)
        seen.append(("a3r_prep_pointmap", depth, float(focal), tables, crop, out))
        return out

    def prep_resize3(src, tables, crop=None):
        out = rs(src, tables, crop)
        seen.append(("a3r_prep_resize3", src, None, tables, crop, out))
        return out

    monkeypatch.setattr(ops, "prep_pointmap", prep_pointmap)
    monkeypatch.setattr(ops, "prep_resize3", prep_resize3)
    return seen


def replay_in_arena(name, src, focal, tables, crop, fill=-777.25):
    """The C call itself with the output and the workspace inside guarded arenas; returns (out, guards intact)."""
    from align3r_amd import _lib
    lib = _lib.load()
    Hs, Ws = src.shape[:2]
    d = tables.desc(Hs, Ws, (0, 0, tables.Hr, tables.Wr) if crop is None else crop)
    need = int(lib.a3r_prep_workspace_bytes(Hs, Ws, d.Wc))
    n = d.Hc * d.Wc * 3
    out = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    ws = torch.full((GUARD + need + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    args = (C.byref(d), ws.data_ptr() + GUARD, need, out.data_ptr() + 4 * GUARD, _lib.stream_ptr())
    rc = lib.a3r_prep_pointmap(src.data_ptr(), focal, *args) if name == "a3r_prep_pointmap" else lib.a3r_prep_resize3(src.data_ptr(), *args)
    torch.cuda.synchronize()
    assert rc == 0, lib.a3r_last_error()
    intact = bool((out[:GUARD] == fill).all() and (out[-GUARD:] == fill).all() and (ws[:GUARD] == 0xAB).all() and (ws[-GUARD:] == 0xAB).all())
    return out[GUARD:GUARD + n].reshape(d.Hc, d.Wc, 3), intact


@pytest.mark.parametrize("name", list(pc.CASES))
def test_pointmap_vs_host(calls, name):
    H, W, size, square_ok, crop = pc.CASES[name]
    img, depth, focal = pc.make_inputs(H, W)
    want_img, want = pc.host_pointmap(img, depth, focal, size, square_ok, crop)
    got_img, got = device_pointmap(img, depth, focal, size, square_ok, crop)
    assert got_img.size == want_img.size and np.array_equal(np.array(got_img), np.array(want_img))
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == pc.OUT_SHAPES[name] + (3,)
    assert pc.same(got.cpu().numpy(), want)
    assert [c[0] for c in calls] == (["a3r_prep_pointmap"] if crop else ["a3r_prep_pointmap", "a3r_prep_resize3"])
    assert calls[0][3].taps == (4 if name in ("14x20_s32", "60x100_s224") else 8) and (crop or calls[1][3].taps == 4)
    # the C calls again on buffers of the test: nothing outside the output and the workspace is written, every output element is,
    # and the bits are the first run's
    for cname, src, f, tables, window, first in calls:
        again, intact = replay_in_arena(cname, src, f, tables, window)
        assert intact and not (again == -777.25).any()
        assert np.array_equal(again.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32))


def test_square_image_without_square_ok_raises_as_the_host_path():
    img, depth, focal = pc.make_inputs(40, 40)
    for crop in (True, False):
        with pytest.raises(TypeError):
            pc.host_pointmap(img, depth, focal, 32, False, crop)
        with pytest.raises(TypeError):
            device_pointmap(img, depth, focal, 32, False, crop)


def _special(depth, kind):
    d = depth.copy()
    H, W = d.shape
    if kind == "nan":
        d[H // 3, W // 2 + 3] = np.nan
    elif kind == "inf":
        d[H - 2, 5] = np.inf
    elif kind == "inf_centre_column":                   # px - W/2 == 0 there when W is even: 0 * inf
        d[H // 2 + 1, W // 2] = np.inf
    elif kind == "constant":
        d[:] = 2.5
    elif kind == "zeros":
        d[::3, 1::4] = 0.0
    elif kind == "all_zero":
        d[:] = 0.0
    return d


@pytest.mark.parametrize("shape", ["37x53_s32", "40x40_s32_square"])
@pytest.mark.parametrize("kind", ["nan", "inf", "inf_centre_column", "constant", "zeros", "all_zero"])
def test_special_values(kind, shape):
    H, W, size, square_ok, crop = pc.CASES[shape]
    img, depth, focal = pc.make_inputs(H, W)
    depth = _special(depth, kind)
    want = pc.host_pointmap(img, depth, focal, size, square_ok, crop)[1]
    got = device_pointmap(img, depth, focal, size, square_ok, crop)[1].cpu().numpy()
    assert pc.same(got, want)
    if kind == "nan":
        assert np.isnan(got).all()                      # one NaN pixel: every channel's min and max, so everything
    if kind == "constant":
        assert np.isnan(got[..., 2]).all() and np.isfinite(got[..., :2]).all()
    if kind == "zeros":
        assert np.isfinite(got).all()
    if kind == "all_zero":
        assert np.isnan(got).all()


@pytest.mark.parametrize("focal", [np.asarray(431.7, dtype=np.float32), 200, np.float64(1e-3), -57.25])
def test_focal_forms(focal):
    H, W, size, square_ok, crop = pc.CASES["23x61_s48"]
    img, depth, _ = pc.make_inputs(H, W)
    want = pc.host_pointmap(img, depth, focal, size, square_ok, crop)[1]
    assert pc.same(device_pointmap(img, depth, focal, size, square_ok, crop)[1].cpu().numpy(), want)


@pytest.mark.parametrize("H,W", [(16, 32), (7, 9)])
def test_image_side(H, W):
    """16 x 32: the 16-byte form; 7 x 9: H * W is no multiple of 4.  Exact-black pixels, channel sums of 2/255 (false) and 3/255 (true)."""
    from align3r_amd import ops
    from align3r_amd.dust3r.utils.image_pose import ImgNorm, ToTensor
    import PIL.Image
    a = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[0, :4] = 0
    a[1, 0], a[1, 1], a[1, 2], a[1, 3] = (1, 1, 0), (0, 0, 2), (1, 1, 1), (0, 3, 0)
    a[2, 0], a[2, 1] = (2, 0, 0), (255, 255, 255)
    a[H - 1, W - 1] = (0, 1, 1)
    pil = PIL.Image.fromarray(a)
    want_img, want_mask = ImgNorm(pil).numpy(), (~(ToTensor(pil)[None].sum(1) <= 0.01))[0].numpy()
    assert not want_mask[0, :4].any() and want_mask[1, :4].tolist() == [False, False, True, True] and not want_mask[H - 1, W - 1]
    G = GUARD
    img = torch.full((G + 3 * H * W + G,), -777.25, dtype=torch.float32, device="cuda")
    mask = torch.full((G + H * W + G,), 0x5A, dtype=torch.uint8, device="cuda")
    from align3r_amd import _lib
    u8 = torch.from_numpy(a).cuda()
    rc = _lib.load().a3r_prep_image(u8.data_ptr(), H, W, img.data_ptr() + 4 * G, mask.data_ptr() + G, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((img[:G] == -777.25).all() and (img[-G:] == -777.25).all() and (mask[:G] == 0x5A).all() and (mask[-G:] == 0x5A).all())
    got_img, got_mask = img[G:-G].reshape(3, H, W).cpu().numpy(), mask[G:-G].reshape(H, W).cpu().numpy()
    assert np.array_equal(got_img.view(np.uint32), want_img.view(np.uint32))
    assert set(np.unique(got_mask).tolist()) <= {0, 1} and np.array_equal(got_mask.astype(bool), want_mask)
    w_img, w_mask = ops.prep_image(u8)
    assert w_img.dtype == torch.float32 and w_mask.dtype == torch.bool and tuple(w_img.shape) == (3, H, W) and tuple(w_mask.shape) == (H, W)
    assert np.array_equal(w_img.cpu().numpy().view(np.uint32), want_img.view(np.uint32)) and np.array_equal(w_mask.cpu().numpy(), want_mask)


def test_bad_arguments_write_nothing():
    """A refusal on real device buffers leaves the output and the workspace untouched (the refusals themselves: test_prep_device_cpu)."""
    from align3r_amd import _lib, ops
    from align3r_amd.dust3r.utils.image_pose import resize_tables
    lib = _lib.load()
    Hs, Ws = 37, 53
    tables = ops.PrepTables(resize_tables(Ws, 32, True), resize_tables(Hs, 22, True), "cuda")
    depth = torch.from_numpy(pc.make_inputs(Hs, Ws)[1]).cuda()
    need = int(lib.a3r_prep_workspace_bytes(Hs, Ws, 32))
    out = torch.full((GUARD + 16 * 32 * 3 + GUARD,), -777.25, dtype=torch.float32, device="cuda")
    ws = torch.full((GUARD + need + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    keep = tables.idx_y[4, 1]
    for over, focal, ws_bytes, msg in ((dict(taps=5), 40.0, need, "taps"), (dict(y0=9), 40.0, need, "crop window"), ({}, 0.0, need, "focal"),
                                       ({}, 40.0, need - 16, "workspace too small"), ("table", 40.0, need, "idx_y[4, 1]")):
        d = tables.desc(Hs, Ws, (3, 0, 16, 32))
        if over == "table":
            tables.idx_y[4, 1] = Hs
        else:
            for k, v in over.items():
                setattr(d, k, v)
        rc = lib.a3r_prep_pointmap(depth.data_ptr(), focal, C.byref(d), ws.data_ptr() + GUARD, ws_bytes, out.data_ptr() + 4 * GUARD, _lib.stream_ptr())
        torch.cuda.synchronize()
        tables.idx_y[4, 1] = keep
        assert rc == -1 and msg in lib.a3r_last_error().decode(), (msg, lib.a3r_last_error())
        assert bool((out == -777.25).all() and (ws == 0xAB).all()), msg
    with pytest.raises(RuntimeError, match="crop window"):
        ops.prep_pointmap(depth, 40.0, tables, (8, 0, 16, 32))


def test_load_images_on_the_device_equals_the_host_path(tmp_path):
    """Three frames (a plain float32 prior, a [1, H, W] one, a float64 one that takes the host functions): view by view the host path's
    numbers, and the views go through collate_with_cat and a .to(device) round as inference() does them."""
    from align3r_amd.dust3r.inference import _IGNORE_KEYS
    from align3r_amd.dust3r.utils.device import collate_with_cat
    from align3r_amd.dust3r.utils.image_pose import load_images
    folder = pc.write_clip(tmp_path)
    kw = dict(verbose=False, traj_format="custom", dynamic_mask_root=str(tmp_path / "none"))
    host, raw_h = load_images(folder, 32, **kw)
    dev, raw_d = load_images(folder, 32, prep_device="cuda", **kw)
    twice, _ = load_images(folder, 32, prep_device="cuda", **kw)
    assert len(host) == len(dev) == len(raw_h) == len(raw_d) == 3
    for h, d, t in zip(host, dev, twice):
        assert set(h) == set(d)
        for key in ("img", "pred_depth", "mask"):
            want = h[key] if isinstance(h[key], np.ndarray) else h[key].numpy()
            assert isinstance(d[key], torch.Tensor) and d[key].is_cuda and tuple(d[key].shape) == want.shape, key
            assert pc.same(d[key].cpu().numpy(), want), key
            assert torch.equal(d[key].view(torch.uint8), t[key].view(torch.uint8)), key                 # two runs, the same bits
        assert d["dynamic_mask"].device.type == "cpu" and torch.equal(d["dynamic_mask"], h["dynamic_mask"])
        assert isinstance(d["true_shape"], np.ndarray) and np.array_equal(d["true_shape"], h["true_shape"])
        assert d["idx"] == h["idx"] and d["instance"] == h["instance"]
    pairs = [(dev[0], dev[1]), (dev[1], dev[2])]
    ref = [(host[0], host[1]), (host[1], host[2])]
    for (v1, v2), (h1, h2) in zip([collate_with_cat(pairs)], [collate_with_cat(ref)]):
        for view, hview in ((v1, h1), (v2, h2)):
            for name in view:
                if name in _IGNORE_KEYS:
                    continue
                moved = view[name].to("cuda", non_blocking=True)
                assert moved.is_cuda and pc.same(moved.cpu().numpy(), hview[name].numpy()), name
    with pytest.raises(NotImplementedError):
        load_images([str(tmp_path / "clip.mp4")], 32, prep_device="cuda", **kw)
