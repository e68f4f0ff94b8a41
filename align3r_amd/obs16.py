"""Packed fp16 pair observations of the aligner (a3r_align_desc.obs_format = 1): the format, written down in numpy.

One edge side is a row of points pred [P, 3] fp32 with its weights w [P] fp32.  Packed, it is one int32 exponent k and P records of
four fp16 values {x 2^k, y 2^k, z 2^k, w}:

    m = max |v| over the FINITE components of pred
    k = 0                                     if m == 0 or the row has no finite component
      = clamp(14 - ilogb(m), -100, 100)       otherwise: the largest finite magnitude lands in [2^14, 2^15), rounds to <= 32768

The scaling by 2^k is exact (ldexp), the conversion rounds to nearest even, non-finite values convert by the IEEE rule.  Decoded,
pred' = float(h) 2^-k and w' = float(h_w) are exact fp32 numbers with |pred' - pred| <= max(2^-11 |pred|, 2^-25 2^-k) (fp16's
11-bit significand and its 2^-24 subnormal step).  The packed aligner IS the fp32 aligner run on (pred', w').

csrc/obs.hip (a3r_align_pack_obs) computes the same on the device, bit for bit; this module is what the tests compare it with.
"""
from __future__ import annotations

import numpy as np

OBS_DTYPES = ("fp32", "fp16")


def check_obs_dtype(obs_dtype):
    if obs_dtype not in OBS_DTYPES:
        raise ValueError(f"obs_dtype must be one of {OBS_DTYPES}, got {obs_dtype!r}")
    return obs_dtype


def row_exponents(pred):
    """k [rows] int32 of pred [rows, P, 3] fp32 by the rule above."""
    pred = np.asarray(pred, dtype=np.float32)
    a = np.abs(pred.reshape(pred.shape[0], -1))
    m = np.where(np.isfinite(a), a, np.float32(0)).max(axis=1)
    _, e = np.frexp(m)                                  # m = f 2^e, f in [0.5, 1): ilogb(m) = e - 1 (subnormals included)
    return np.where(m > 0, np.clip(14 - (e - 1), -100, 100), 0).astype(np.int32)


def pack_reference(pred, w):
    """(records [rows, P, 4] float16, exponents [rows] int32) of pred [rows, P, 3] and w [rows, P]."""
    pred = np.asarray(pred, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    k = row_exponents(pred)
    with np.errstate(over="ignore", invalid="ignore"):
        rec = np.empty(pred.shape[:2] + (4,), np.float16)
        rec[..., :3] = np.ldexp(pred, k[:, None, None]).astype(np.float16)
        rec[..., 3] = w.astype(np.float16)
    return rec, k


def decode(rec, k):
    """(pred' [rows, P, 3], w' [rows, P]) fp32 of packed records: float(h) 2^-k, float(h_w)."""
    rec = np.asarray(rec, dtype=np.float16)
    f = rec.astype(np.float32)
    with np.errstate(invalid="ignore"):
        pred = np.ldexp(f[..., :3], -np.asarray(k, dtype=np.int32)[:, None, None])
    return pred.astype(np.float32), np.ascontiguousarray(f[..., 3])
