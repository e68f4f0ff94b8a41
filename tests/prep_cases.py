"""Shared by tests/test_prep_device_cpu.py and tests/test_gpu_prep.py: seeded priors and images, the host yardstick (the package's own
pixel_to_pointcloud / crop_img / ImgNorm), the arithmetic contract of csrc/prep.hip restated in numpy, and a folder of frames with priors."""
import numpy as np
import PIL.Image

# name -> (H, W, size, square_ok, crop): the cases of the device path (heights x widths of the prior and of the image)
CASES = {
    "37x53_s32": (37, 53, 32, False, True),            # 8 taps, replicated borders, a 16 x 32 window of a 22 x 32 map
    "14x20_s32": (14, 20, 32, False, True),            # 4-tap enlarge
    "23x61_s48": (23, 61, 48, False, True),            # odd sizes on both axes, 16 rows out of 18
    "37x53_s32_nocrop": (37, 53, 32, False, False),    # second cubic resize from the rounded float32 map
    "60x100_s224": (60, 100, 224, False, True),        # short-side rule, square centre crop
    "40x40_s32_square": (40, 40, 32, True, True),      # the accepted square branch
    "436x1024_s512": (436, 1024, 512, False, True),    # the one realistic shape
}
OUT_SHAPES = {"37x53_s32": (16, 32), "14x20_s32": (16, 32), "23x61_s48": (16, 48), "37x53_s32_nocrop": (16, 32), "60x100_s224": (224, 224),
              "40x40_s32_square": (32, 32), "436x1024_s512": (208, 512)}


def make_inputs(H, W, seed=0):
    """(PIL image W x H, depth float32 [H, W], focal as the float32 0-d array an .npz holds)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = (1.5 + 2.0 * ys + np.sin(5 * xs) + 0.3 * rng.random((H, W))).astype(np.float32)
    img = PIL.Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return img, depth, np.asarray(0.9 * max(H, W), dtype=np.float32)


def host_pointmap(img, depth, focal, size, square_ok, crop):
    """The yardstick: what load_images does for the point map of one frame."""
    from align3r_amd.dust3r.utils.image_pose import crop_img, pixel_to_pointcloud
    with np.errstate(all="ignore"):
        return crop_img(img, size, pixel_to_pointcloud(depth, focal), square_ok=square_ok, crop=crop)


def same(a, b):
    """Equal as numbers, NaNs in the same places (the sign of a zero is not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def apply_tables(src, x_tab, y_tab):
    """The separable resample as the kernels do it: float64, tap 0 first, every product and sum rounded, horizontal then vertical."""
    (ix, wx), (iy, wy) = x_tab, y_tab
    src = src.astype(np.float64)
    mid = np.zeros((src.shape[0], len(ix)) + src.shape[2:], np.float64)
    for k in range(ix.shape[1]):
        mid = mid + src[:, ix[:, k]] * wx[:, k].reshape((1, -1) + (1,) * (src.ndim - 2))
    out = np.zeros((len(iy),) + mid.shape[1:], np.float64)
    for k in range(iy.shape[1]):
        out = out + mid[iy[:, k]] * wy[:, k].reshape((-1,) + (1,) * (src.ndim - 1))
    return out


def contract_pointmap(depth, focal, x_tab, y_tab, window):
    """DESIGN 6.7 in numpy, scalar order of operations: un-project in float64, round, min / max, normalise in float32, resample."""
    Hs, Ws = depth.shape
    f = np.float64(focal)
    with np.errstate(all="ignore"):
        d = depth.astype(np.float64)
        x = (((np.arange(Ws, dtype=np.float64) - Ws / 2)[None, :] * d) / f).astype(np.float32)
        y = (((np.arange(Hs, dtype=np.float64) - Hs / 2)[:, None] * d) / f).astype(np.float32)
        pts = np.stack((x, y, depth), -1)
        mn, mx = pts.min((0, 1)), pts.max((0, 1))
        norm = ((pts - mn) / (mx - mn)).astype(np.float32)
        y0, x0, Hc, Wc = window
        out = apply_tables(norm, (x_tab[0][x0:x0 + Wc], x_tab[1][x0:x0 + Wc]), (y_tab[0][y0:y0 + Hc], y_tab[1][y0:y0 + Hc]))
    return out.astype(np.float32)


def write_clip(folder, n=3, H=30, W=44, seed=5):
    """n PNG frames with .npz priors under the 'custom' naming rule: frame 0 a plain float32 prior, frame 1 a [1, H, W] one, frame 2 a
    float64 one (the device path hands that frame to the host functions).  Returns the folder as a string."""
    for k in range(n):
        img, depth, focal = make_inputs(H, W, seed + k)
        img.save(folder / f"frame_{k:02d}.png")
        if k == 1:
            depth = depth[None]
        if k == 2:
            depth = depth.astype(np.float64)
        np.savez(folder / f"frame_{k:02d}_pred_depth_depthpro.npz", depth=depth, focallength_px=focal)
    return str(folder)
