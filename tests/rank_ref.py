"""The definition of nm_transform_draws (include/nuts_amd.h) restated in numpy — a helper, not a test: the pool, the fold, the
keys (quantile_ref's), a sort of the keys, the counts a and b by binary search, rank2 = a + b + 1; the indicator; and the composition
rank_diagnostics makes of them with summary_ref and quantile_ref.  The device's rank2, NaN counts and indicator equal this BIT FOR BIT
(tests/test_gpu_rank.py): they are integer counts and one comparison.  The score of a rank is the library's host twin
nm_rank_normal_score — the same header the kernel compiles, no device needed; score_numpy is the same algorithm transcribed with
libm's logarithm, which may differ from it in the last bits."""
import ctypes as C

import numpy as np

import quantile_ref
import summary_ref

RANK_NORMAL, FOLDED_RANK_NORMAL, INDICATOR_LE = 0, 1, 2

PA = (3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
      4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
PB = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
      2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
PC = (1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
      1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
PD = (1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
      1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
PE = (6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
PF = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
      7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    p = np.float64(c[7])
    for k in range(6, -1, -1):
        p = p * r + np.float64(c[k])
    return p


def score_numpy(n, rank2):
    """the header's algorithm for one (n, rank2), every step one binary64 operation, with libm's log in place of dlog"""
    A, B = 4 * int(rank2) - 3, 8 * int(n) + 2
    q = np.float64(2 * A - B) / np.float64(2 * B)
    if abs(q) <= 0.425:
        r = np.float64(0.180625) - q * q
        return q * _horner(PA, r) / _horner(PB, r)
    t = np.float64(min(A, B - A)) / np.float64(B)
    r = np.sqrt(-np.log(t))
    if r <= 5.0:
        r = r - np.float64(1.6)
        w = _horner(PC, r) / _horner(PD, r)
    else:
        r = r - np.float64(5.0)
        w = _horner(PE, r) / _horner(PF, r)
    return -w if q < 0 else w


def score_twin(n, rank2):
    """nm_rank_normal_score over an array of rank2 (one call per distinct value)"""
    import nuts_rs_amd as N
    L = N.load_library()
    r = np.asarray(rank2, dtype=np.uint64)
    uniq, inv = np.unique(r.reshape(-1), return_inverse=True)
    z = C.c_double()
    vals = np.empty(len(uniq))
    for i, u in enumerate(uniq.tolist()):
        assert L.nm_rank_normal_score(int(n), int(u), C.byref(z)) == 0, (n, u)
        vals[i] = z.value
    return vals[inv].reshape(r.shape)


def pool_draws(n_draws, split):
    """the draws in the pool: all of them, without the middle one when the trace is split and n_draws is odd"""
    rows = np.arange(n_draws)
    return rows[rows != n_draws // 2] if (split and n_draws % 2 == 1) else rows


def _select(draws, chain_ids):
    x = np.ascontiguousarray(draws, dtype=np.float64)
    assert x.ndim == 3
    return x if chain_ids is None else np.ascontiguousarray(x[:, np.asarray(chain_ids, dtype=np.int64), :])


def column_rank2(v):
    """rank2 of the values of one pool (any shape): a = keys below, b = keys not above, a + b + 1"""
    k = quantile_ref.keys(np.asarray(v, dtype=np.float64).reshape(-1))
    s = np.sort(k)
    a, b = np.searchsorted(s, k, side="left"), np.searchsorted(s, k, side="right")
    return (a + b + 1).astype(np.uint32).reshape(np.shape(v))


def transform(draws, kind, param=None, split=True, chain_ids=None):
    """(out [N][C'][D], rank2 uint32 [N][C'][D] or None, nan_count uint64 [D]) of draws [N][C][D]"""
    x = _select(draws, chain_ids)
    N, Cs, D = x.shape
    if kind == INDICATOR_LE:
        c = np.asarray(param, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            out = np.where(x <= c, 1.0, 0.0)
        out[np.isnan(x)] = np.nan
        out[:, :, np.isnan(c)] = np.nan
        return out, None, np.isnan(x).sum(axis=(0, 1)).astype(np.uint64)
    rows = pool_draws(N, split)
    n = len(rows) * Cs
    v = x[rows]
    if kind == FOLDED_RANK_NORMAL:
        with np.errstate(invalid="ignore"):
            v = np.abs(v - np.asarray(param, dtype=np.float64))          # one subtraction, then the sign bit cleared
    nan_count = np.isnan(v).sum(axis=(0, 1)).astype(np.uint64)
    rank2 = np.zeros((N, Cs, D), dtype=np.uint32)
    out = np.full((N, Cs, D), np.nan)
    for d in range(D):
        if nan_count[d]:
            continue
        rank2[rows, :, d] = column_rank2(v[:, :, d])
        out[rows, :, d] = score_twin(n, rank2[rows, :, d])
    return out, rank2, nan_count


def rank_diagnostics(draws, split=True, max_lag=32, chain_ids=None):
    """what nuts_rs_amd.rank_diagnostics composes, from the three restatements"""
    from types import SimpleNamespace
    q, _ = quantile_ref.quantile(draws, [0.05, 0.5, 0.95], chain_ids=chain_ids)
    z, _, nan_count = transform(draws, RANK_NORMAL, None, split, chain_ids)
    bulk = summary_ref.summarize(z, split, max_lag)
    folded = summary_ref.summarize(transform(draws, FOLDED_RANK_NORMAL, q[1], split, chain_ids)[0], split, max_lag)
    lower = summary_ref.summarize(transform(draws, INDICATOR_LE, q[0], split, chain_ids)[0], split, max_lag)
    upper = summary_ref.summarize(transform(draws, INDICATOR_LE, q[2], split, chain_ids)[0], split, max_lag)
    with np.errstate(invalid="ignore"):
        return SimpleNamespace(rhat_rank=np.maximum(bulk.rhat, folded.rhat), ess_bulk=bulk.ess, ess_tail=np.minimum(lower.ess, upper.ess),
                               ess_bulk_truncated=bulk.ess_truncated, ess_tail_truncated=lower.ess_truncated | upper.ess_truncated,
                               nan_count=nan_count)


DIAG_FIELDS = ("rhat_rank", "ess_bulk", "ess_tail", "ess_bulk_truncated", "ess_tail_truncated", "nan_count")
