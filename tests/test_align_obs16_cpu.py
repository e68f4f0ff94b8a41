"""CPU: the packed fp16 observation format of the aligner (align3r_amd/obs16.py, the written definition that csrc/obs.hip is
compared with on the GPU) -- exponent rule, finiteness, the format's error bound, idempotence -- and the ABI / keyword surface.

The bound |pred' - pred| <= max(2^-11 |pred|, 2^-25 2^-k) is the format's: fp16 has an 11-bit significand (half an ulp is 2^-11
relative) and a 2^-24 subnormal step (half of it, 2^-25, in the scaled domain, 2^-25 2^-k after decoding)."""
import numpy as np
import pytest

from align3r_amd import obs16

P = 1028


def row_kinds(P=P, seed=5):
    """(pred [7, P, 3], w [7, P]): the seven row kinds the format was checked on.  Row 6 holds inf and nan."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((7, P, 3)).astype(np.float32)
    x[1] *= np.float32(1e6)
    x[2] *= np.float32(1e-30)
    x[3] = np.clip(x[3], -7.5, 7.5)
    x[3, 17, 1] = 8.0                                          # maximum exactly 8: k = 11, lands on 2^14
    x[4] = np.clip(x[4], -7.5, 7.5)
    x[4, 5, 2] = -np.nextafter(np.float32(8), np.float32(0))   # rounds to 32768, finite
    x[5] = 0.0
    x[6, 3, 0], x[6, 9, 1], x[6, 11, 2] = np.inf, np.nan, -np.inf
    w = np.log1p(9 * rng.random((7, P))).astype(np.float32)
    return x, w


def _ilogb(m):
    return int(np.floor(np.log2(float(m))))


def test_exponent_rule():
    x, w = row_kinds()
    rec, k = obs16.pack_reference(x, w)
    assert rec.dtype == np.float16 and rec.shape == (7, P, 4) and k.dtype == np.int32 and k.shape == (7,)
    for r in range(7):
        fin = np.abs(x[r][np.isfinite(x[r])])
        m = fin.max() if fin.size else 0.0
        want = 0 if m == 0 else int(np.clip(14 - _ilogb(m), -100, 100))
        assert k[r] == want, (r, k[r], want)
        if m > 0 and abs(want) < 100:
            assert 2.0 ** 14 <= float(m) * 2.0 ** want < 2.0 ** 15
    assert k[3] == 11 and k[4] == 12 and k[5] == 0 and k[2] == 100
    assert np.abs(rec[3, :, :3].astype(np.float32)).max() == 16384.0
    assert np.abs(rec[4, :, :3].astype(np.float32)).max() == 32768.0       # nextafter(8, 0) 2^12 rounds up, and is finite
    assert np.array_equal(rec[5, :, :3].view(np.uint16), np.zeros((P, 3), np.uint16))
    # an all-non-finite row has k = 0
    bad = np.full((1, 8, 3), np.nan, np.float32)
    assert obs16.pack_reference(bad, np.ones((1, 8), np.float32))[1][0] == 0


def test_finite_stays_finite_and_error_bound():
    x, w = row_kinds()
    rec, k = obs16.pack_reference(x, w)
    xd, wd = obs16.decode(rec, k)
    assert xd.dtype == np.float32 and wd.dtype == np.float32 and xd.shape == x.shape and wd.shape == w.shape
    fin = np.isfinite(x)
    assert np.isfinite(xd[fin]).all()
    assert np.array_equal(np.isnan(xd), np.isnan(x)) and np.array_equal(np.isposinf(xd), np.isposinf(x))
    assert np.array_equal(np.isneginf(xd), np.isneginf(x))
    x64, xd64 = x.astype(np.float64), xd.astype(np.float64)
    bound = np.maximum(2.0 ** -11 * np.abs(x64), 2.0 ** -25 * np.ldexp(1.0, -k.astype(np.int64))[:, None, None])
    assert (np.abs(xd64[fin] - x64[fin]) <= bound[fin]).all()
    assert np.array_equal(wd, w.astype(np.float16).astype(np.float32))
    assert (np.abs(wd.astype(np.float64) - w) <= 2.0 ** -11 * np.abs(w) + 2.0 ** -25).all()


def test_pack_of_decoded_is_identity():
    x, w = row_kinds()
    rec, k = obs16.pack_reference(x, w)
    xd, wd = obs16.decode(rec, k)
    rec2, k2 = obs16.pack_reference(xd, wd)
    xd2, wd2 = obs16.decode(rec2, k2)
    assert np.array_equal(xd2.view(np.uint32), xd.view(np.uint32)) and np.array_equal(wd2.view(np.uint32), wd.view(np.uint32))


def test_align_desc_has_the_packed_fields_zero_by_default():
    from align3r_amd._lib import AlignDesc
    names = [f[0] for f in AlignDesc._fields_]
    assert names[-5:] == ["obs_format", "obs_i", "obs_j", "obs_exp_i", "obs_exp_j"]
    assert names[-6] == "adam_pw_adaptors"
    d = AlignDesc()
    assert d.obs_format == 0 and not d.obs_i and not d.obs_j and not d.obs_exp_i and not d.obs_exp_j


@pytest.mark.parametrize("cls", ["AlignEngine", "ShardedAlignEngine"])
def test_unknown_obs_dtype_is_refused_before_any_device_work(cls, monkeypatch):
    import align3r_amd._lib as _lib
    import align3r_amd.aligner as aligner

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before obs_dtype was checked")
    monkeypatch.setattr(_lib, "load", no_device)
    x, w = row_kinds(32)
    kw = dict(local_shards=1) if cls == "ShardedAlignEngine" else {}
    with pytest.raises(ValueError, match="obs_dtype"):
        getattr(aligner, cls)([0, 1], [1, 0], x[:2], x[2:4], w[:2], w[2:4], [(4, 8)] * 2, obs_dtype="bf16", **kw)
    with pytest.raises(ValueError, match="obs_dtype"):
        obs16.check_obs_dtype("bf16")
    assert obs16.check_obs_dtype("fp16") == "fp16" and obs16.check_obs_dtype("fp32") == "fp32"
