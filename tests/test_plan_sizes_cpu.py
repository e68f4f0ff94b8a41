"""CPU (no GPU): the sizing passes of the two launch plans report exactly the packed-buffer and workspace sizes recorded in
golden/plan_sizes.json, which was written from the commit before the plans moved onto the shared core (csrc/plan.h); the flow
network's last three shapes were added from the commit before its plan was split into stages.  Workspace
layout is observable (a fixed call sequence on a fresh handle is reproducible), so a changed size means a moved,
added or resized allocation."""
import importlib.util
import json
import os

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_plan_sizes", os.path.join(GOLDEN, "make_goldens_plan_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_sizes_match_the_recorded_ones():
    gen = _generator()
    want = json.load(open(os.path.join(GOLDEN, "plan_sizes.json")))
    got = gen.measure()
    # 2 configs x 7 modes x (packed + 5 shapes x {forward, encode}) + 2 flow configs x (packed + 6 shapes)
    assert len(want) == 2 * len(gen.MODES) * (1 + 2 * len(gen.MODEL_SHAPES)) + 2 * (1 + len(gen.RAFT_SHAPES)) == 168
    assert set(got) == set(want)
    assert all(v > 0 for v in want.values())
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
