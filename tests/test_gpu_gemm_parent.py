"""GPU: the three matrix-kernel families (csrc/gemm.hip, gemm_bf3.hip, gemm_fh2.hip) compute, bit for bit, what the commit before
their tile scaffold, conv geometry, epilogue preamble, launch helper and entry checks were shared computed: y, every auxiliary output
and the out_absmax word, per family and per forced tile, on full and ragged tiles, 1-5 k-stages, every epilogue and output form,
grouped launches, the arithmetic modes, the conv shapes that reach every border and stage count, and A3R_BF3_DIRECT_EPI=1.
tests/golden/gemm_parent.json was written by tests/golden/make_goldens_gemm_parent.py from that commit's library; the cases and how
one is measured are imported from there.  No tolerance: SHA-256 digests, compared for equality.  Seeded numpy inputs, at most 300 rows."""
import importlib.util
import json
import os
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_gemm_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_gemm_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _generator()
_child_ended_badly = False


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "gemm_parent.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(_PARENT.CASES) and len(golden) == 59
    assert all(len(rec) >= 4 and all(len(d) == 64 for d in rec.values()) for rec in golden.values())


@pytest.mark.parametrize("name", list(_PARENT.CASES))          # the case that needs a child process is the last one
def test_gemm_bitwise_parent(name, golden, tmp_path):
    """Any non-zero status of a child process raises; after one, nothing more is started on the GPU from this file."""
    global _child_ended_badly
    assert not _child_ended_badly, "not started: an earlier child process of this file ended abnormally"
    try:
        got = _PARENT.measure_case(name, str(tmp_path))
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        _child_ended_badly = _child_ended_badly or "child process" in str(e) or isinstance(e, subprocess.TimeoutExpired)
        raise
    want = golden[name]
    assert got == want, (name, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k)))
