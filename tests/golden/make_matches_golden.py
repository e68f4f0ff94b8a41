#!/usr/bin/env python3
"""Generate tests/golden/matches.npz by RUNNING THE REFERENCE's find_reciprocal_matches and xy_grid (dust3r/utils/geometry.py).

Usage (where a checkout of the reference is present):  python tests/golden/make_matches_golden.py REFERENCE_DIR

The reference module is imported from REFERENCE_DIR and called; none of its text is stored.  Per case c of CASES (clouds of
tests/match_cases.py, P1 seed 11, P2 seed 12): P1_c, P2_c float32 and the three outputs reciprocal_c bool [n2], nn2_c int64 [n2],
count_c.  xy_grid: grid_np (W=5, H=3), grid_origin (W=4, H=2, origin=(3, 7)), grid_homog (W=3, H=2, homogeneous=True) from the numpy
branch, and grid_torch (W=6, H=4, device='cpu') and grid_planes (W=3, H=2, device='cpu', unsqueeze=0, cat_dim=None: the two planes
stacked for storage) from the torch branch."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import match_cases as mc  # noqa: E402

CASES = [("surface", 1000, 1337), ("uniform", 65, 257)]


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "dust3r", "utils", "geometry.py")):
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from dust3r.utils.geometry import find_reciprocal_matches, xy_grid
    out = {}
    for c, (kind, n1, n2) in enumerate(CASES):
        P1, P2 = mc.pair(kind, n1, n2)
        rec, nn2, count = find_reciprocal_matches(P1, P2)
        out[f"P1_{c}"], out[f"P2_{c}"] = P1, P2
        out[f"reciprocal_{c}"], out[f"nn2_{c}"], out[f"count_{c}"] = np.asarray(rec, bool), np.asarray(nn2, np.int64), np.int64(count)
    out["grid_np"] = xy_grid(5, 3)
    out["grid_origin"] = xy_grid(4, 2, origin=(3, 7))
    out["grid_homog"] = xy_grid(3, 2, homogeneous=True)
    out["grid_torch"] = xy_grid(6, 4, device="cpu").numpy()
    gx, gy = xy_grid(3, 2, device="cpu", unsqueeze=0, cat_dim=None)
    out["grid_planes"] = np.stack([gx.numpy(), gy.numpy()])
    np.savez_compressed(os.path.join(HERE, "matches.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
