#!/usr/bin/env python3
"""Generate tests/golden/depth_eval.npz by RUNNING THE REFERENCE's LAD scale / shift (tool/depth_test.py: absolute_error_loss,
absolute_value_scaling) on three small float32 clips of tests/depth_eval_cases.py.

Usage (where a checkout of the reference is present):  python tests/golden/make_goldens_depth_eval.py REFERENCE_DIR

tool/depth_test.py cannot be imported (it pulls in cv2 and third-party models at import time), so the two functions are compiled
one by one from its syntax tree, as make_goldens.py does for the other single functions; no reference source text is stored.  The
call is the reference's (:724-725): the valid pixels as float32 tensors, started at torch.median(gt) / torch.median(pred).
Stored per clip k: pred_k, gt_k [3, 24, 32] float32 and st_k = the reference's (s, t) as float64."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
SHAPE = (3, 24, 32)
FAMILIES = ("lognormal", "cauchy", "sqrt")


def _ref_function(ref, path, name, glb):
    src = open(os.path.join(ref, path)).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.join(ref, path), "exec"), glb)
            return glb[name]
    raise KeyError(name)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "tool", "depth_test.py")):
        sys.exit(__doc__)
    ref = sys.argv[1]
    import torch
    from scipy.optimize import minimize
    import depth_eval_cases as dc
    glb = dict(np=np, torch=torch, minimize=minimize)
    _ref_function(ref, "tool/depth_test.py", "absolute_error_loss", glb)
    scaling = _ref_function(ref, "tool/depth_test.py", "absolute_value_scaling", glb)
    out = {}
    for k, fam in enumerate(FAMILIES):
        pred, gt = dc.make_clip(fam, SHAPE)
        with np.errstate(invalid="ignore"):
            valid = np.logical_and(gt > 1e-3, gt < dc.DEPTH_MAX)
        p, g = torch.from_numpy(pred[valid]), torch.from_numpy(gt[valid])
        s, t = scaling(p, g, s=torch.median(g) / torch.median(p))
        out[f"pred_{k}"], out[f"gt_{k}"], out[f"st_{k}"] = pred, gt, np.array([s, t], np.float64)
        print(fam, "reference (s, t) =", float(s), float(t))
    np.savez_compressed(os.path.join(HERE, "depth_eval.npz"), **out)


if __name__ == "__main__":
    main()
