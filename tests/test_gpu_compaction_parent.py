"""GPU: the entries built on the count / scan / place compaction (csrc/scene.hip point cloud and mesh, voxel.hip, match.hip, the
surface of tsdf.hip, the 'scale' rule of metrics.hip) compute, bit for bit, what the commit before the workgroup rank, the scan
kernel and the host epilogue were shared (csrc/compact.h) computed: every output of every call, on shapes below a wave, at exactly
one chunk, one past it, with ragged and padded images, with all / none / one / half of the items kept, and at 1024 * 1024 + 1025
items, where a thread of the scan owns two chunk counts.  tests/golden/compaction_parent.json was written by
tests/golden/make_goldens_compaction_parent.py from that commit's library (two runs of it gave the same file); the cases and how one
is measured are imported from there.  No tolerance: SHA-256 digests, compared for equality."""
import importlib.util
import json
import os

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_compaction_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_compaction_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _generator()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "compaction_parent.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(_PARENT.CASES) and len(golden) == 31
    assert all(len(rec) >= 1 and all(len(d) == 64 for d in rec.values()) for rec in golden.values())
    # the masks do select: within a scene case the four point clouds differ, and so do the single- and the double-sided mesh
    for name, rec in golden.items():
        if name.startswith("scene/"):
            assert len({rec[f"{m}/points"] for m in ("all", "none", "one", "half")}) == 4, name
            assert rec["all/mesh1"] != rec["all/mesh2"], name


@pytest.mark.parametrize("name", list(_PARENT.CASES))
def test_compaction_bitwise_parent(name, golden):
    got = _PARENT.measure_case(name)
    want = golden[name]
    assert got == want, (name, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k)))
