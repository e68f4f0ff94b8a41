"""Host-side helpers of the renderer (ops.render_points, csrc/render.hip): the one place where a camera pose is inverted, and the PNG
writer of scene.save_renders.  The reference looks at an aligned scene through interactive viewers (scene.show(), tool/demo.py);
on a machine without a display the scene is rendered into pictures instead."""
from __future__ import annotations

import numpy as np


def world_to_camera(cam2world):
    """The rigid inverse [R^T | -R^T t] of camera-to-world poses [..., 3 or 4, 4], in float64 numpy: [..., 3, 4] world-to-camera
    transforms as ops.render_points takes them.  Torch tensors (any device) are accepted."""
    if hasattr(cam2world, "detach"):
        cam2world = cam2world.detach().cpu().numpy()
    c2w = np.asarray(cam2world, dtype=np.float64)
    if c2w.ndim < 2 or c2w.shape[-1] != 4 or c2w.shape[-2] not in (3, 4):
        raise ValueError(f"world_to_camera: poses are [..., 3 or 4, 4], got {c2w.shape}")
    R, t = c2w[..., :3, :3], c2w[..., :3, 3]
    Rt = np.swapaxes(R, -1, -2)
    return np.concatenate([Rt, -(Rt @ t[..., None])], axis=-1)


def write_png(path, rgb):
    """An [H, W, 3] (or [H, W]) uint8 picture as a PNG through PIL, which the image loader already requires."""
    import PIL.Image
    if hasattr(rgb, "detach"):
        rgb = rgb.detach().cpu().numpy()
    arr = np.ascontiguousarray(rgb)
    if arr.dtype != np.uint8 or not (arr.ndim == 2 or (arr.ndim == 3 and arr.shape[2] == 3)):
        raise ValueError(f"write_png: an [H, W, 3] or [H, W] uint8 array is needed, got {arr.dtype} {arr.shape}")
    PIL.Image.fromarray(arr).save(path, format="PNG")
    return path
