#!/usr/bin/env python3
"""Input preprocessing, host path against device path in one process (developer tool): load_images on folders of synthetic frames
with mono-depth priors of 436 x 1024 (Sintel) and 1080 x 1920 (the davis rule; 480 x 854 images), size 512, 16 frames.  Per frame:
the stages of the host path (un-project + normalise, resize + crop of the map, ImgNorm + mask) and of the device path (upload of the
depth map; one a3r_prep_pointmap call: four kernels, workspace and output allocation included, 20 calls per timing; upload of the
uint8 image + a3r_prep_image), each the median of repeats after a warm-up and ended by a device synchronise; then the whole of
load_images both ways (PIL decode and resize and the .npz read are in both).
The host path is the parent commit's code, unchanged by the device path.  The two results are compared for equality.

    python tools/bench_prep.py [--frames 16] [--repeats 5] [--out profiles/prep_device.json]
"""
import argparse, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, PIL.Image, torch
from align3r_amd import ops
from align3r_amd.dust3r.utils import image_pose as ip

SIZE = 512
SHAPES = [((436, 1024), (436, 1024)), ((1080, 1920), (480, 854))]          # (prior, image), heights x widths


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def write_frames(folder, n, prior_hw, image_hw):
    rng = np.random.default_rng(0)
    (Hp, Wp), (Hi, Wi) = prior_hw, image_hw
    ys, xs = np.meshgrid(np.linspace(0, 1, Hp), np.linspace(0, 1, Wp), indexing="ij")
    for k in range(n):
        depth = (1.5 + 2.0 * ys + np.sin(5 * xs + k) + 0.3 * rng.random((Hp, Wp))).astype(np.float32)
        PIL.Image.fromarray(rng.integers(0, 256, (Hi, Wi, 3), dtype=np.uint8)).save(os.path.join(folder, f"f{k:03d}.png"))
        np.savez(os.path.join(folder, f"f{k:03d}_pred_depth_depthpro.npz"), depth=depth, focallength_px=np.float32(0.9 * Wp))


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "prep_device.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for prior_hw, image_hw in SHAPES:
        with tempfile.TemporaryDirectory() as folder:
            write_frames(folder, a.frames, prior_hw, image_hw)
            kw = dict(verbose=False, traj_format="custom", dynamic_mask_root=os.path.join(folder, "none"), interval=a.frames)
            t_host, (host, _) = timed(lambda: ip.load_images(folder, SIZE, **kw), 3)
            t_dev, (devv, _) = timed(lambda: ip.load_images(folder, SIZE, prep_device=dev, **kw), 3)
            equal = all(np.array_equal(d[k].cpu().numpy(), np.asarray(h[k]), equal_nan=True) for h, d in zip(host, devv)
                        for k in ("img", "pred_depth", "mask"))
            # the stages, on frame 0
            path = os.path.join(folder, "f000.png")
            raw = PIL.Image.open(path).convert("RGB")
            t_npz, prior = timed(lambda: dict(np.load(path.replace(".png", "_pred_depth_depthpro.npz"))), a.repeats)
            depth, focal = prior["depth"], prior["focallength_px"]
            t_pil, (img, _) = timed(lambda: ip.crop_img(raw, SIZE), a.repeats)
            t_unproject, pts = timed(lambda: ip.pixel_to_pointcloud(depth, focal), a.repeats)
            ref = ip.crop_img(raw, SIZE, pts)[1]
            Hc, Wc = ref.shape[:2]
            t_resample, again = timed(lambda: ip.crop_center(ip.resize_numpy_image(pts, SIZE), Wc, Hc), a.repeats)
            assert np.array_equal(again, ref, equal_nan=True)
            t_imgnorm, _ = timed(lambda: (ip.ImgNorm(img)[None], ~(ip.ToTensor(img)[None].sum(1) <= 0.01)), a.repeats)
            t_upload, d_dev = timed(lambda: torch.from_numpy(depth).to(dev), a.repeats)
            Hp, Wp = prior_hw
            (Wr, Hr), lanczos = ip._numpy_resize_plan(Hp, Wp, SIZE)
            tables = ip._device_tables(Hp, Wp, Hr, Wr, bool(lanczos), str(dev))
            window = (Hr // 2 - Hc // 2, Wr // 2 - Wc // 2, Hc, Wc)
            assert np.array_equal(ops.prep_pointmap(d_dev, float(focal), tables, window).cpu().numpy(), ref, equal_nan=True)

            def kernels(n=20):
                for _ in range(n):
                    ops.prep_pointmap(d_dev, float(focal), tables, window)

            t_kernels = timed(kernels, a.repeats)[0] / 20
            u8 = np.array(img, copy=True)
            t_img_dev, _ = timed(lambda: ops.prep_image(torch.from_numpy(u8).to(dev)), a.repeats)
            nbytes = 2 * Hp * Wp * 4 + 2 * Hp * Wc * 24 + Hc * Wc * 12          # depth read twice, the intermediate written and read, the map written
            results.append(dict(prior=list(prior_hw), image=list(image_hw), size=SIZE, frames=a.frames, out=[int(Hc), int(Wc)], results_equal=bool(equal),
                                load_images_host_s_per_frame=t_host / a.frames, load_images_device_s_per_frame=t_dev / a.frames,
                                npz_read_s=t_npz, pil_resize_crop_s=t_pil, host_unproject_normalise_s=t_unproject,
                                host_resample_crop_s=t_resample, host_imgnorm_mask_s=t_imgnorm,
                                device_upload_depth_s=t_upload, device_pointmap_call_s=t_kernels,
                                device_image_upload_and_kernel_s=t_img_dev, upload_bytes=int(depth.nbytes), kernel_bytes=int(nbytes)))
            print(json.dumps(results[-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_prep.py", device=torch.cuda.get_device_name(0), torch_threads=torch.get_num_threads(), results=results), f, indent=1)


if __name__ == "__main__":
    main()
