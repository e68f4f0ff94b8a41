#!/usr/bin/env python3
"""Generate tests/golden/mesh.npz (+ mesh.json) by RUNNING THE REFERENCE's mesh construction (dust3r/viz.py: pts3d_to_trimesh,
cat_meshes -- what get_3D_model_from_scene calls with as_pointcloud=False) on small masks.

Usage (where a checkout of the reference is present):  python tests/golden/make_goldens_mesh.py REFERENCE_DIR

dust3r/viz.py imports trimesh and matplotlib-side helpers at import time; the two functions need numpy alone, so they are compiled
one by one from the file's syntax tree, as make_goldens.py does for other single functions; no reference source text is stored.
The call is the reference's: meshes = [pts3d_to_trimesh(img_n, pts_n, valid_n)], cat_meshes(meshes), images as float [h,w,3] in
[0, 1].  Stored per case c and image n: valid_c_n bool [h,w], img_c_n uint8 [h,w,3] (the float image is img / 255), and per case
faces_c int32 [F,3] (indices into the concatenated DENSE grids: image offsets = cumulative h * w) and colors_c uint8 [F,3] =
rint(255 * face_colors).  The point maps do not enter the faces; random ones are passed and not stored."""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# name: list of (h, w, kept fraction); 1.0 / 0.0 = a fully kept / fully dropped image
CASES = {
    "three_6x7": [(6, 7, 0.7)] * 3,
    "mixed_6x8_8x6": [(6, 8, 0.7), (8, 6, 0.7)],
    "full_and_empty": [(6, 7, 1.0), (6, 7, 0.0), (6, 7, 0.7)],
    "full_5x7": [(5, 7, 1.0)],
}


def _ref_function(ref, path, name, glb):
    src = open(os.path.join(ref, path)).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.join(ref, path), "exec"), glb)
            return glb[name]
    raise KeyError(name)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "dust3r", "viz.py")):
        sys.exit(__doc__)
    ref = sys.argv[1]
    glb = dict(np=np)
    to_trimesh = _ref_function(ref, "dust3r/viz.py", "pts3d_to_trimesh", glb)
    cat = _ref_function(ref, "dust3r/viz.py", "cat_meshes", glb)
    rng = np.random.default_rng(20)
    out, meta = {}, {}
    for c, (name, images) in enumerate(CASES.items()):
        meshes = []
        for n, (h, w, frac) in enumerate(images):
            valid = rng.random((h, w)) < frac
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            pts = rng.standard_normal((h, w, 3)).astype(np.float32)
            out[f"valid_{c}_{n}"], out[f"img_{c}_{n}"] = valid, img
            meshes.append(to_trimesh(img.astype(np.float32) / 255, pts, valid))
        mesh = cat(meshes)
        out[f"faces_{c}"] = mesh["faces"].astype(np.int32).reshape(-1, 3)
        out[f"colors_{c}"] = np.rint(255 * mesh["face_colors"]).astype(np.uint8).reshape(-1, 3)
        meta[name] = dict(case=c, shapes=[[h, w] for h, w, _ in images], kept=[int(out[f"valid_{c}_{n}"].sum()) for n in range(len(images))],
                          faces=int(len(out[f"faces_{c}"])))
    assert meta["full_5x7"]["faces"] == 4 * 4 * 6            # every quad of a full 5x7 image: 4 triangles each
    np.savez_compressed(os.path.join(HERE, "mesh.npz"), **out)
    with open(os.path.join(HERE, "mesh.json"), "w") as f:
        json.dump(dict(cases=meta, note="faces / colors: cat_meshes(pts3d_to_trimesh(...)) of the reference's dust3r/viz.py"), f, indent=1)
        f.write("\n")
    print({k: v["faces"] for k, v in meta.items()})


if __name__ == "__main__":
    main()
