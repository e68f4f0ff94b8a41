"""GPU: the two kernel forms of the bilinear 2x (csrc/elementwise.hip) are bitwise equal.
The second form (default) makes 2 x 2 output pixels per thread from corners fetched once; the first form (A3R_UP_FORM=v1 /
a3r_upsample2x_set_form(1)) fetches four corners per output pixel and is the reference.  Every entry point that has two forms is
compared byte for byte, the fh2 range word included: fp32 output, fh2 output, and the combine pass of the DPT heads."""
import ctypes as C

import pytest
import torch

from align3r_amd import _lib

pytestmark = pytest.mark.gpu

# (B, H, W, C, crop): the 2x2 blocks start at output -1, so an even and an odd window end differently on each axis
SHAPES = [
    (2, 3, 5, 8, None),
    (2, 3, 5, 8, (5, 10)),           # crop to (2H - 1, 2W)
    (2, 3, 5, 8, (5, 9)),
    (2, 3, 5, 8, (2, 1)),
    (2, 1, 5, 8, None),              # H = 1: both source rows are row 0
    (2, 4, 1, 16, None),             # W = 1
    (1, 1, 1, 8, None),
    (1, 6, 8, 128, None),
    (2, 4, 6, 256, None),
    (1, 9, 20, 128, (17, 40)),       # two workgroups along x; 9 block rows, more than the workgroups along y: the row loop repeats
]


@pytest.fixture(scope="module")
def ops():
    from align3r_amd import ops as o
    return o


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 3).cuda()


def both_forms(run):
    """run() under form 1, then under form 2; the process-wide switch is put back."""
    lib = _lib.load()
    prev = lib.a3r_upsample2x_set_form(2)
    assert prev in (1, 2)
    try:
        outs = []
        for form in (1, 2):
            assert lib.a3r_upsample2x_set_form(form) in (1, 2)
            outs.append(run())
    finally:
        lib.a3r_upsample2x_set_form(prev)
    return outs


@pytest.mark.parametrize("B,H,W,Cc,crop", SHAPES)
def test_fp32_forms_are_bitwise_equal(ops, B, H, W, Cc, crop):
    x = rnd(B, H, W, Cc, seed=H * 100 + W)

    def run():
        Hc, Wc = crop if crop else (2 * H, 2 * W)
        out = torch.full((B, Hc, Wc, Cc), float("nan"), device="cuda")
        rc = _lib.load().a3r_upsample2x(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), B, H, W, Cc, Hc, Wc, _lib.stream_ptr())
        assert rc == 0
        return out
    v1, v2 = both_forms(run)
    assert not torch.isnan(v1).any()
    assert torch.equal(v1, v2)


@pytest.mark.parametrize("B,H,W,Cc,crop", SHAPES)
def test_fh2_forms_are_bitwise_equal(ops, B, H, W, Cc, crop):
    x = rnd(B, H, W, Cc, seed=H * 100 + W + 1)

    def run():
        word = ops.absmax_word("cuda")
        out = ops.upsample2x_fh2(x, crop=crop, scale=4.0, absmax=word)
        return out.data.clone(), int(word.item())
    (d1, w1), (d2, w2) = both_forms(run)
    assert w1 > 0
    assert torch.equal(d1, d2)
    assert w1 == w2


@pytest.mark.parametrize("S,U,H,W,Cc,crop,idx", [
    (3, 2, 3, 5, 8, (5, 10), [1, 1, 0]),           # U < S, a map that repeats
    (4, 2, 4, 6, 256, None, [0, 1, 1, 0]),
    (2, 1, 1, 1, 16, None, [0, 0]),
    (3, 3, 9, 20, 128, (17, 39), [2, 0, 1]),
])
def test_combine_forms_are_bitwise_equal(ops, S, U, H, W, Cc, crop, idx):
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    x, c, r0 = rnd(S, H, W, Cc, seed=7), rnd(U, Hc, Wc, Cc, seed=8), rnd(U, Hc, Wc, Cc, seed=9)
    m = torch.tensor(idx, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def run():
        s = torch.full((S, Hc, Wc, Cc), float("nan"), device="cuda")
        sr2 = torch.zeros(S * Hc * Wc * Cc * 4, dtype=torch.uint8, device="cuda")
        word = ops.absmax_word("cuda")
        rc = _lib.load().a3r_upsample2x_combine_fh2(p(x), p(c), p(r0), p(m), p(s), p(sr2), S, H, W, Cc, Hc, Wc, 2.0, p(word),
                                                    _lib.stream_ptr())
        assert rc == 0
        return s, sr2, int(word.item())
    (s1, q1, w1), (s2, q2, w2) = both_forms(run)
    assert not torch.isnan(s1).any() and w1 > 0
    assert torch.equal(s1, s2)
    assert torch.equal(q1, q2)
    assert w1 == w2
    # the first form itself: the RESID2 order of additions on the fp32 form's map
    up = ops.upsample2x(x, crop=(Hc, Wc))
    assert torch.equal(s1, c[m.long()] + (r0[m.long()] + up))
