"""GPU: the pair network's launch plan (csrc/model.hip: run_plan and its stages) computes, bit for bit, what the commit before the
plan was split into stages -- and before the fp32 DPT head moved onto the operand-form path -- computed: every output, the fh2
site scales and statistics (so the order of the sites), and what was merged, in every arithmetic mode, with duplicate inputs,
through encode / decode, and under every switch that selects another path of the plan.  tests/golden/model_parent.json was written
by tests/golden/make_goldens_model_parent.py from that commit's library; the cases and how one is measured are imported from there.
No tolerance: SHA-256 digests and tuples, compared for equality.  TINY config, synthetic weights, at most five pairs of 64x96."""
import importlib.util
import json
import os
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_model_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_model_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _generator()
_child_ended_badly = False


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "model_parent.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(_PARENT.CASES) and len(golden) == 36


@pytest.mark.parametrize("name", list(_PARENT.CASES))          # the cases that need a child process are the last ones
def test_plan_bitwise_parent(name, golden, tmp_path):
    """Any non-zero status of a child process raises; after one, nothing more is started on the GPU from this file."""
    global _child_ended_badly
    assert not _child_ended_badly, "not started: an earlier child process of this file ended abnormally"
    try:
        got = _PARENT.measure_case(name, str(tmp_path))
    except (RuntimeError, subprocess.TimeoutExpired):
        _child_ended_badly = True
        raise
    want = golden[name]
    assert ("encode" in want and "decode" in want) or {"pts3d_1", "conf_2", "site_scales", "site_stats", "last_dedup_sides"} <= set(want)
    assert got == want, (name, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
