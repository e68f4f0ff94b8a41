"""CPU: the host side of the device preprocessing path (csrc/prep.hip).  The factored-out table builder applied in numpy is
cv2_resize; the arithmetic contract of the kernels restated in numpy is the host path; a3r_prep_* refuse bad arguments from the host
copies of their tables before they touch the device; load_images without prep_device is the host path."""
import ctypes as C

import numpy as np
import pytest
import torch

import prep_cases as pc


@pytest.mark.parametrize("shape,new_size,lanczos", [((37, 53, 3), (32, 22), True), ((14, 20, 3), (32, 22), False), ((23, 61), (48, 18), True),
                                                    ((9, 7, 3), (7, 31), False), ((40, 12, 3), (5, 40), True)])
def test_tables_applied_in_numpy_are_cv2_resize(shape, new_size, lanczos):
    """Lanczos shrink, cubic enlarge, both axes (and one axis shrinking while the other grows under one filter)."""
    from align3r_amd.dust3r.utils.image_pose import cv2_resize, resize_tables
    src = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    w, h = new_size
    x_tab, y_tab = resize_tables(shape[1], w, lanczos), resize_tables(shape[0], h, lanczos)
    taps = 8 if lanczos else 4
    for (idx, wt), n, new_len in ((x_tab, shape[1], w), (y_tab, shape[0], h)):
        assert idx.shape == wt.shape == (new_len, taps) and wt.dtype == np.float64 and idx.min() >= 0 and idx.max() <= n - 1
        assert (np.diff(idx, axis=0) >= 0).all() and (np.diff(idx, axis=1) >= 0).all()
    want = cv2_resize(src, new_size, lanczos)
    assert pc.same(pc.apply_tables(src, x_tab, y_tab).astype(np.float32), want)


@pytest.mark.parametrize("name", ["37x53_s32", "14x20_s32", "23x61_s48", "40x40_s32_square"])
def test_contract_in_numpy_is_the_host_path(name):
    """DESIGN 6.7's order of operations, written out: the same numbers as crop_img(pixel_to_pointcloud(...)) on the crop window."""
    from align3r_amd.dust3r.utils.image_pose import _numpy_resize_plan, resize_tables
    H, W, size, square_ok, crop = pc.CASES[name]
    img, depth, focal = pc.make_inputs(H, W)
    _, want = pc.host_pointmap(img, depth, focal, size, square_ok, crop)
    assert want.shape[:2] == pc.OUT_SHAPES[name]
    (Wr, Hr), lanczos = _numpy_resize_plan(H, W, size)
    Hc, Wc = want.shape[:2]
    window = (Hr // 2 - Hc // 2, Wr // 2 - Wc // 2, Hc, Wc)
    got = pc.contract_pointmap(depth, focal, resize_tables(W, Wr, lanczos), resize_tables(H, Hr, lanczos), window)
    assert pc.same(got, want)
    got = pc.contract_pointmap(depth, 200, resize_tables(W, Wr, lanczos), resize_tables(H, Hr, lanczos), window)
    assert pc.same(got, pc.host_pointmap(img, depth, 200, size, square_ok, crop)[1])


def test_c_calls_validate_on_the_host_before_any_launch():
    """Every refusal of a3r_prep_pointmap / a3r_prep_resize3 / a3r_prep_image comes before the device is touched: no GPU is needed."""
    from align3r_amd import _lib
    from align3r_amd.dust3r.utils.image_pose import resize_tables
    lib = _lib.load()
    Hs, Ws, Hr, Wr, taps = 37, 53, 22, 32, 8
    ix, wx = resize_tables(Ws, Wr, True)
    iy, wy = resize_tables(Hs, Hr, True)
    ix, iy = np.ascontiguousarray(ix, dtype=np.int32), np.ascontiguousarray(iy, dtype=np.int32)
    need = int(lib.a3r_prep_workspace_bytes(Hs, Ws, 32))
    assert need >= Hs * 32 * 3 * 8 and need % 16 == 0
    for empty in ((0, Ws, 32), (Hs, 0, 32), (Hs, Ws, 0), (-1, Ws, 32)):
        assert lib.a3r_prep_workspace_bytes(*empty) == 0
    fake = 1 << 20                                            # stands for a device pointer: never dereferenced on these paths

    def call(fn="a3r_prep_pointmap", src=fake, focal=40.0, ws=fake, ws_bytes=need, out=fake, **over):
        f = dict(Hs=Hs, Ws=Ws, Hr=Hr, Wr=Wr, taps=taps, y0=3, x0=0, Hc=16, Wc=32, idx_x=fake, idx_x_host=ix.ctypes.data, w_x=fake, idx_y=fake,
                 idx_y_host=iy.ctypes.data, w_y=fake)
        f.update(over)
        d = C.byref(_lib.PrepDesc(**f))
        if fn == "a3r_prep_pointmap":
            rc = lib.a3r_prep_pointmap(src, focal, d, ws, ws_bytes, out, None)
        else:
            rc = lib.a3r_prep_resize3(src, d, ws, ws_bytes, out, None)
        return rc, lib.a3r_last_error().decode()

    refusals = [(dict(src=None), "null source or output"), (dict(out=None), "null source or output"), (dict(idx_x=None), "null index or weight"),
                (dict(w_y=None), "null index or weight"), (dict(idx_y_host=None), "null index or weight"), (dict(ws=None), "workspace too small"),
                (dict(ws_bytes=need - 1), "workspace too small"), (dict(ws=fake + 8), "16-byte aligned"), (dict(Hs=0), "must be positive"),
                (dict(Ws=-2), "must be positive"), (dict(Hc=0), "must be positive"), (dict(Wc=-1), "must be positive"),
                (dict(Hr=0), "must be positive"), (dict(taps=6), "taps"), (dict(taps=0), "taps"), (dict(y0=7), "crop window"),
                (dict(x0=1), "crop window"), (dict(y0=-1), "crop window"), (dict(Hc=23, y0=0), "crop window"),
                (dict(w_x=fake + 4), "tables must be 16-byte aligned")]
    for fn in ("a3r_prep_pointmap", "a3r_prep_resize3"):
        for kw, msg in refusals:
            rc, err = call(fn, **kw)
            assert rc == -1 and msg in err and fn in err, (fn, kw, err)
    for focal in (0.0, -0.0, float("nan"), float("inf"), float("-inf")):
        rc, err = call(focal=focal)
        assert rc == -1 and "focal" in err, (focal, err)
    for tab, name, bad in ((ix, "idx_x", Ws), (ix, "idx_x", -1), (iy, "idx_y", Hs), (iy, "idx_y", -1)):
        keep = tab[5, 2]
        tab[5, 2] = bad
        for fn in ("a3r_prep_pointmap", "a3r_prep_resize3"):
            rc, err = call(fn)
            assert rc == -1 and f"{name}[5, 2]" in err, (name, bad, err)
        tab[5, 2] = keep
    for kw, msg in ((dict(u8=None), "null image"), (dict(img=None), "null image"), (dict(mask=None), "null image"), (dict(H=0), "must be positive"),
                    (dict(W=-4), "must be positive")):
        f = dict(u8=fake, H=16, W=32, img=fake, mask=fake)
        f.update(kw)
        rc = lib.a3r_prep_image(f["u8"], f["H"], f["W"], f["img"], f["mask"], None)
        assert rc == -1 and msg in lib.a3r_last_error().decode(), kw


def test_wrappers_refuse_host_tensors():
    from align3r_amd import ops
    with pytest.raises(RuntimeError, match="float32 CUDA tensor"):
        ops.prep_pointmap(torch.zeros(4, 4), 1.0, None)
    with pytest.raises(RuntimeError, match="float32 CUDA tensor"):
        ops.prep_resize3(torch.zeros(4, 4, 3), None)
    with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
        ops.prep_image(torch.zeros(4, 4, 3, dtype=torch.uint8))


def test_load_images_without_prep_device_is_the_host_path(tmp_path):
    from align3r_amd.dust3r.utils.image_pose import crop_img, load_images
    from align3r_amd.tool import run_clip
    folder = pc.write_clip(tmp_path)
    views, raws = load_images(folder, 32, verbose=False, traj_format="custom", dynamic_mask_root=str(tmp_path / "none"), prep_device=None)
    again, _ = load_images(folder, 32, verbose=False, traj_format="custom", dynamic_mask_root=str(tmp_path / "none"))
    assert len(views) == len(raws) == 3
    for k, (v, w) in enumerate(zip(views, again)):
        assert isinstance(v["pred_depth"], np.ndarray) and v["pred_depth"].dtype == np.float32 and v["pred_depth"].shape == (1, 16, 32, 3)
        assert v["img"].device.type == "cpu" and v["img"].dtype == torch.float32 and tuple(v["img"].shape) == (1, 3, 16, 32)
        assert v["mask"].device.type == "cpu" and v["mask"].dtype == torch.bool and v["dynamic_mask"].dtype == torch.bool
        assert v["idx"] == k and v["true_shape"].tolist() == [[16, 32]]
        assert pc.same(v["pred_depth"], w["pred_depth"]) and torch.equal(v["img"], w["img"])
    img, depth, focal = pc.make_inputs(37, 53)
    a, b = crop_img(img, 32, None, device=None), crop_img(img, 32)
    assert a[1] is None and b[1] is None and a[0].size == b[0].size == (32, 16)
    base = ["--images", "x", "--weights", "y", "--out", "z"]
    assert run_clip.parse(base).device_prep is False and run_clip.parse(base + ["--device-prep"]).device_prep is True
