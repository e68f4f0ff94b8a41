"""GPU: the attention kernels (csrc/attention.hip, attention_bf3.hip, attention_fh2.hip: both forms and the single-pass mode) compute,
bit for bit, what the commit before their placement, softmax step, product ladders, staged operands, epilogue, entry checks and
launch were shared (csrc/attention_tile.h) computed: the output and, for fh2, the out_absmax word, on every shape of
attention_refs.SHAPES with ten (batch, head) groups per launch, at products 6 / 3 / 1 and both bf3 output layouts, in both fh2 forms
at scale 1 and at the scaled set, in the single-pass mode, through image maps, on column-sliced operands and at 1, 7, 8, 9 and 17
groups.  tests/golden/attention_parent.json was written by tests/golden/make_goldens_attention_parent.py from that commit's library
(two runs of it gave the same file); the cases and how one is measured are imported from there.  No tolerance: SHA-256 digests,
compared for equality."""
import importlib.util
import json
import os

import pytest

import test_gpu_attention_f64 as F64
from conftest import REPO

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_attention_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_attention_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _generator()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "attention_parent.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(_PARENT.CASES) and len(golden) == 55
    assert all(len(rec) >= 1 and all(len(d) == 64 for d in rec.values()) for rec in golden.values())
    assert (_PARENT.SCALED_MUL, _PARENT.SCALED) == (F64.SCALED_MUL, F64.SCALED)


@pytest.mark.parametrize("name", list(_PARENT.CASES))
def test_attention_bitwise_parent(name, golden):
    got = _PARENT.measure_case(name)
    want = golden[name]
    assert got == want, (name, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k)))
