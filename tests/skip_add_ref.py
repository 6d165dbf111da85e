"""The ControlNet skip add bit for bit on the CPU: one correctly rounded fp32 fma per live source, then one rounding to the
destination's type.  numpy has no fp32 fma; fma32 gets one out of fp64 by rounding the sum to odd before the cast."""
import numpy as np


def fma32(s, a, v):
    """the correctly rounded fp32 fma(s, a, v) of fp32 arrays.  p = s a is exact in fp64 (24 + 24 bits).  t = fl64(p + v) alone would round twice
    (to 53 bits, then to 24) and lands on the wrong side where the first rounding produces a midpoint of fp32; so t is rounded to odd instead:
    TwoSum gives the error of the fp64 sum exactly, an inexact t is truncated towards zero and its lowest bit set.  53 >= 24 + 2 bits: the cast
    to fp32 then rounds as if from the exact sum."""
    s, a, v = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (s, a, v))
    with np.errstate(invalid="ignore", over="ignore"):
        p = s * a
        t = p + v
        vv = t - p
        err = (p - (t - vv)) + (v - vv)      # TwoSum: p + v == t + err exactly
        inexact = np.isfinite(t) & (err != 0)
        towards_zero = inexact & ((err < 0) == (t > 0))
        bits = np.atleast_1d(t).view(np.int64).copy()      # (sign-magnitude: one less is one fp64 towards zero; an inexact t is never 0)
        bits[np.atleast_1d(towards_zero)] -= 1
        bits[np.atleast_1d(inexact)] |= 1
        return bits.view(np.float64).reshape(np.shape(t)).astype(np.float32)


def skip_add_expected(dst, srcs, scales, dtype, skip_zero=True):
    """the bits the add leaves in dst [rows, C] under one scale per source: f = fp32(dst); for k in order, f = fma32(scales[k], fp32(srcs[k]), f);
    the result cast to `dtype` (numpy rounds to nearest even).  skip_zero: a source at scale 0 does not enter (the table forms, where it is not even
    read); False is the one-scalar form, which computes fma(0, src, dst) like any other scale.  Call it per batch entry."""
    f = np.asarray(dst).astype(np.float32)
    for s, a in zip(scales, srcs):
        if skip_zero and np.float32(s) == 0:
            continue
        f = fma32(np.float32(s), np.asarray(a).astype(np.float32), f)
    with np.errstate(over="ignore"):
        return f.astype(dtype)
