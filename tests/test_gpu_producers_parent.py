"""GPU: the memory-bound producers of csrc/elementwise.hip (LayerNorm fp32 / bf3 / fh2, the bilinear 2x in both forms and three
output formats, the residual combine alone and inside the 2x, the gather-add with two sources) and the Umeyama moments kernel of
csrc/init.hip compute, bit for bit, what the commit before their kernels were put on shared helpers computed: every output of every
call, the statistics word and the sentinel bytes a call must leave alone included, on the smallest shapes that reach each launcher
branch and the second trip of each persistent loop.  tests/golden/producers_parent.json was written by
tests/golden/make_goldens_producers_parent.py from that commit's library (two runs of it gave the same file); the cases and how one
is measured are imported from there.  No tolerance: SHA-256 digests, compared for equality."""
import importlib.util
import json
import os

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_goldens_producers_parent",
                                                  os.path.join(REPO, "tests", "golden", "make_goldens_producers_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PARENT = _generator()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "producers_parent.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(_PARENT.CASES) and len(golden) == 46
    assert all(len(rec) >= 1 and all(len(d) == 64 for d in rec.values()) for rec in golden.values())
    # what that commit's own tests pin shows in the file: the two forms of an entry, and the two places a block is read from, gave
    # the same bytes; the statistics word and the scale do reach the digests
    for name, rec in golden.items():
        for tag in {k.rsplit("/form", 1)[0] for k in rec if "/form" in k}:
            assert rec[f"{tag}/form1"] == rec[f"{tag}/form2"], (name, tag)
        if name.startswith("comb/"):
            assert rec["map"] == rec["src"], name
        if name.startswith("upc_src/"):
            assert rec == golden[name.replace("upc_src/", "upc/")], name
        if name.startswith("ln_fh2/"):
            assert len(set(rec.values())) == len(rec), name


@pytest.mark.parametrize("name", list(_PARENT.CASES))
def test_producers_bitwise_parent(name, golden):
    got = _PARENT.measure_case(name)
    want = golden[name]
    assert got == want, (name, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k)))
