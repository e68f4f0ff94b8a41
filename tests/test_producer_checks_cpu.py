"""CPU (no GPU): the entry checks of the producers of csrc/elementwise.hip return A3R_EINVAL with the exact a3r_last_error text,
one bad argument per check: null pointer, bad scale (0, -1, inf, NaN), bad C multiple, crop window too large, misaligned pointer,
bad storage stride.  Every call fails before any HIP call, so the pointers are never followed: they are made-up addresses.  The
expected texts were printed by the library of the commit before the checks were shared (check_scale, check_up2x_shape,
all_aligned16), not derived from the new code; the texts of a3r_upsample2x_combine_fh2 carry no a3r_ prefix, as that commit
printed them."""
import math

import pytest

A, U = 0x10000, 0x10004          # a 16-byte aligned address and one 4 bytes off
EINVAL = -1
BAD_SCALES = (0.0, -1.0, math.inf, math.nan)


def ln_fh2(x=A, w=A, b=A, y2=A, M=4, D=32, scale=1.0):
    return "a3r_layernorm_fh2", (x, w, b, y2, M, D, 1e-6, scale, None, None)


def ln_bf3(y3=A, D=32):
    return "a3r_layernorm_bf3", (A, A, A, y3, 4, D, 1e-6, 1, None)


def gadd(a=A, b=A, dst=A):
    return "a3r_gather_add_rows", (a, A, b, A, dst, 2, 3, 8, None)


def gadd_src(store=A, stride=24, fresh=A, src=A, b=A, dst=A, Cc=8):
    return "a3r_gather_add_rows_src", (store, stride, fresh, src, b, A, dst, 2, 3, Cc, None)


def comb(c=A, r0=A, p2=A, m=A, s=A, sr2=A, Cc=8, scale=1.0):
    return "a3r_combine_resid_fh2", (c, r0, p2, m, s, sr2, 2, 5, Cc, scale, None, None)


def comb_src(c=A, r0=A, sc=A, sr=A, stride=40, src=A, p2=A, s=A, sr2=A, Cc=8, scale=1.0):
    return "a3r_combine_resid_fh2_src", (c, r0, sc, sr, stride, src, p2, s, sr2, 2, 5, Cc, scale, None, None)


def up(name, y=A, Cc=8, Hc=6, Wc=10, x=A):
    return name, (x, y, 2, 3, 5, Cc, Hc, Wc, None)


def up_fh2(x=A, y2=A, Cc=8, Hc=6, Wc=10, scale=1.0):
    return "a3r_upsample2x_fh2", (x, y2, 2, 3, 5, Cc, Hc, Wc, scale, None, None)


def upc(x=A, c=A, r0=A, m=A, s=A, sr2=A, Cc=8, Hc=6, Wc=10, scale=1.0):
    return "a3r_upsample2x_combine_fh2", (x, c, r0, m, s, sr2, 2, 3, 5, Cc, Hc, Wc, scale, None, None)


def upc_src(x=A, c=A, r0=A, sc=A, sr=A, stride=480, src=A, s=A, sr2=A, Cc=8, Hc=6, Wc=10, scale=1.0):
    return "a3r_upsample2x_combine_fh2_src", (x, c, r0, sc, sr, stride, src, s, sr2, 2, 3, 5, Cc, Hc, Wc, scale, None, None)


CHECKS = [
    (ln_fh2(x=None), "a3r_layernorm_fh2: null pointer"),
    (ln_fh2(y2=None), "a3r_layernorm_fh2: null pointer"),
    *[(ln_fh2(scale=v), "a3r_layernorm_fh2: scale must be positive and finite") for v in BAD_SCALES],
    (ln_fh2(D=40), "a3r_layernorm_fh2: bad shape M=4 D=40 (D must be a multiple of 32)"),
    (ln_fh2(y2=U), "a3r_layernorm_fh2: y2 must be 16-byte aligned"),
    (ln_bf3(y3=None), "a3r_layernorm_bf3: null pointer"),
    (ln_bf3(D=12), "a3r_layernorm_bf3: bad shape M=4 D=12 (D must be a multiple of 8)"),
    (ln_bf3(D=40), "a3r_layernorm_bf3: the row-pair layout needs D (40) to be a multiple of 32"),
    (ln_bf3(y3=U), "a3r_layernorm_bf3: y3 must be 16-byte aligned"),
    (gadd(a=None), "a3r_gather_add_rows: null pointer"),
    (gadd(a=U), "a3r_gather_add_rows: buffers must be 16-byte aligned"),
    (gadd(b=U), "a3r_gather_add_rows: buffers must be 16-byte aligned"),
    (gadd(dst=U), "a3r_gather_add_rows: buffers must be 16-byte aligned"),
    (gadd_src(fresh=None), "a3r_gather_add_rows_src: null pointer"),
    (gadd_src(Cc=6), "a3r_gather_add_rows_src: bad shape"),
    (gadd_src(stride=20), "a3r_gather_add_rows_src: bad shape"),
    (gadd_src(stride=26), "a3r_gather_add_rows_src: bad shape"),
    *[(gadd_src(**{k: U}), "a3r_gather_add_rows_src: buffers must be 16-byte aligned") for k in ("store", "fresh", "b", "dst")],
    (comb(p2=None), "a3r_combine_resid_fh2: null pointer"),
    (comb(c=None), "a3r_combine_resid_fh2: null pointer"),
    (comb(Cc=12), "a3r_combine_resid_fh2: bad shape (C must be a multiple of 8)"),
    *[(comb(scale=v), "a3r_combine_resid_fh2: scale must be positive and finite") for v in BAD_SCALES],
    *[(comb(**{k: U}), "a3r_combine_resid_fh2: buffers must be 16-byte aligned") for k in ("c", "r0", "p2", "s", "sr2")],
    (comb_src(src=None), "a3r_combine_resid_fh2_src: null pointer"),
    (comb_src(c=None, r0=None, sc=None, sr=None), "a3r_combine_resid_fh2_src: null pointer"),
    (comb_src(Cc=12), "a3r_combine_resid_fh2_src: bad shape (C must be a multiple of 8)"),
    (comb_src(stride=36), "a3r_combine_resid_fh2_src: bad storage stride or pointers"),
    (comb_src(stride=42), "a3r_combine_resid_fh2_src: bad storage stride or pointers"),
    (comb_src(sc=None), "a3r_combine_resid_fh2_src: bad storage stride or pointers"),
    *[(comb_src(scale=v), "a3r_combine_resid_fh2_src: scale must be positive and finite") for v in BAD_SCALES],
    *[(comb_src(**{k: U}), "a3r_combine_resid_fh2_src: buffers must be 16-byte aligned") for k in ("c", "r0", "sc", "sr", "p2", "s", "sr2")],
    (up("a3r_upsample2x", x=None), "a3r_upsample2x: null pointer"),
    (up("a3r_upsample2x", Cc=6), "a3r_upsample2x: bad shape"),
    (up("a3r_upsample2x", Hc=7), "a3r_upsample2x: crop window larger than the 2x map"),
    (up("a3r_upsample2x", Wc=11), "a3r_upsample2x: crop window larger than the 2x map"),
    (up("a3r_upsample2x", Hc=0), "a3r_upsample2x: crop window larger than the 2x map"),
    (up("a3r_upsample2x_bf3", y=None), "a3r_upsample2x_bf3: null pointer"),
    (up("a3r_upsample2x_bf3", Cc=12), "a3r_upsample2x_bf3: bad shape (C must be a multiple of 8)"),
    (up("a3r_upsample2x_bf3", Wc=11), "a3r_upsample2x_bf3: crop window larger than the 2x map"),
    (up_fh2(y2=None), "a3r_upsample2x_fh2: null pointer"),
    *[(up_fh2(scale=v), "a3r_upsample2x_fh2: scale must be positive and finite") for v in BAD_SCALES],
    (up_fh2(Cc=12), "a3r_upsample2x_fh2: bad shape (C must be a multiple of 8)"),
    (up_fh2(Hc=7), "a3r_upsample2x_fh2: crop window larger than the 2x map"),
    (upc(m=None), "upsample2x_combine_fh2: null pointer"),
    *[(upc(scale=v), "upsample2x_combine_fh2: scale must be positive and finite") for v in BAD_SCALES],
    (upc(Cc=12), "upsample2x_combine_fh2: bad shape (C must be a multiple of 8)"),
    (upc(Wc=11), "upsample2x_combine_fh2: crop window larger than the 2x map"),
    *[(upc(**{k: U}), "upsample2x_combine_fh2: buffers must be 16-byte aligned") for k in ("x", "c", "r0", "s", "sr2")],
    (upc_src(s=None), "a3r_upsample2x_combine_fh2_src: null pointer"),
    *[(upc_src(scale=v), "a3r_upsample2x_combine_fh2_src: scale must be positive and finite") for v in BAD_SCALES],
    (upc_src(Cc=12), "a3r_upsample2x_combine_fh2_src: bad shape (C must be a multiple of 8)"),
    (upc_src(Hc=7), "a3r_upsample2x_combine_fh2_src: crop window larger than the 2x map"),
    (upc_src(stride=476), "a3r_upsample2x_combine_fh2_src: bad storage stride or pointers"),
    (upc_src(stride=482), "a3r_upsample2x_combine_fh2_src: bad storage stride or pointers"),
    (upc_src(r0=None), "a3r_upsample2x_combine_fh2_src: bad storage stride or pointers"),
    *[(upc_src(**{k: U}), "a3r_upsample2x_combine_fh2_src: buffers must be 16-byte aligned") for k in ("x", "c", "r0", "sc", "sr", "s", "sr2")],
]


@pytest.mark.parametrize("i", range(len(CHECKS)))
def test_entry_check_text(i):
    from align3r_amd import _lib
    lib = _lib.load()
    (name, args), text = CHECKS[i]
    assert getattr(lib, name)(*args) == EINVAL, (name, args)
    assert lib.a3r_last_error().decode() == text, (name, args)


def test_set_form_check():
    from align3r_amd import _lib
    lib = _lib.load()
    assert lib.a3r_upsample2x_set_form(3) == EINVAL
    assert lib.a3r_last_error().decode() == "a3r_upsample2x_set_form: form must be 1 or 2"
