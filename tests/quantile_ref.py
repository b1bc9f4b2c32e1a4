"""The definition of nm_quantile_draws (include/nuts_amd.h) restated in numpy, operation by operation: the keys, a sort of
the keys, the ranks h = p (n - 1), lo, g, hi in binary64, and the three operations of the interpolation.  The device result equals this
BIT FOR BIT (tests/test_gpu_quantile.py): it is built from integer counts, so no summation order has to be agreed on."""
import numpy as np

SIGN = np.uint64(0x8000000000000000)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(x):
    """the total order: key(x) = bits(x) ^ (sign ? all ones : the sign bit), compared as unsigned 64-bit"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), ALL, SIGN)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63), SIGN, ALL)).view(np.float64)


def ranks(p, n):
    """(lo, hi, g) of one probability for a pooled sample of n values"""
    h = np.float64(p) * np.float64(n - 1)
    lo = np.floor(h)
    g = h - lo
    lo = int(lo)
    return lo, min(lo + 1, n - 1), g


def quantile(draws, probs, chain_ids=None):
    """(quantiles [n_probs, dim], nan_count [dim] uint64) of draws [n_draws, n_chains, dim]"""
    x = np.ascontiguousarray(draws, dtype=np.float64)
    assert x.ndim == 3
    if chain_ids is not None:
        x = x[:, np.asarray(chain_ids, dtype=np.int64), :]
    dim = x.shape[2]
    x = x.reshape(-1, dim)
    n = x.shape[0]
    k = np.sort(keys(x), axis=0)                       # equal keys are equal bits: any order of ties gives the same x_(r)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    nan_count = np.isnan(x).sum(axis=0).astype(np.uint64)
    out = np.empty((len(probs), dim))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, p in enumerate(probs):
            lo, hi, g = ranks(p, n)
            klo, khi = k[lo], k[hi]
            xlo, xhi = unkeys(klo), unkeys(khi)
            q = xlo + g * (xhi - xlo)                  # one subtraction, one multiplication, one addition
            out[i] = np.where((g == 0.0) | (klo == khi), xlo, q)
    out[:, nan_count > 0] = np.nan
    return out, nan_count
