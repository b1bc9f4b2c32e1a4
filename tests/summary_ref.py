"""The definition of nm_summarize_draws (include/nuts_amd.h) restated in numpy — a helper, not a test.

Every operation is one binary64 + - * or / in the order the header gives, so the device result can be compared bit for bit: the sums
over draws are serial in t (the loops over t and k run in Python, vectorised over series and elements), the sums over series run in
chunks of NM_SUMMARY_CHUNK_CHAINS consecutive series, serially inside a chunk and then over the chunk partials."""
from types import SimpleNamespace

import numpy as np

from nuts_rs_amd import NM_SUMMARY_CHUNK_CHAINS


def chunked_series_sum(a):
    """sum over axis 0 (series): chunks of NM_SUMMARY_CHUNK_CHAINS, serial from 0.0 inside a chunk, partials in chunk order from 0.0"""
    total = np.zeros(a.shape[1:])
    for c0 in range(0, a.shape[0], NM_SUMMARY_CHUNK_CHAINS):
        part = np.zeros(a.shape[1:])
        for m in range(c0, min(c0 + NM_SUMMARY_CHUNK_CHAINS, a.shape[0])):
            part = part + a[m]
        total = total + part
    return total


def summarize(draws, split=True, max_lag=32, chain_ids=None):
    x = np.asarray(draws, dtype=np.float64)
    N, C, D = x.shape
    if chain_ids is not None:
        x = x[:, np.asarray(chain_ids, dtype=np.int64), :]
    if split:
        n = N // 2
        series = np.concatenate([x[:n], x[N - n:]], axis=1)          # [n][M][D]: first halves, then second halves
    else:
        n = N
        series = x
    M = series.shape[1]
    L = min(int(max_lag), n - 1)
    nd, md = float(n), float(M)
    with np.errstate(all="ignore"):
        s = np.zeros((M, D))
        for t in range(n):
            s = s + series[t]
        mean_m = s / nd
        y = series - mean_m                                           # y_t = x_t - mean_m
        acov_m = np.zeros((L + 1, M, D))
        for t in range(n):
            for k in range(0, min(t, L) + 1):
                acov_m[k] = acov_m[k] + y[t] * y[t - k]
        acov_m = acov_m / nd
        var_m = acov_m[0] * nd / (nd - 1.0)
        gm = chunked_series_sum(mean_m) / md
        W = chunked_series_sum(var_m) / md
        dl = mean_m - gm
        Bn = chunked_series_sum(dl * dl) / (md - 1.0)
        var_plus = W * (nd - 1.0) / nd + Bn
        sd = np.sqrt(var_plus)
        rhat = np.sqrt(var_plus / W)
        acov = np.stack([chunked_series_sum(acov_m[k]) for k in range(L + 1)]) / md
        rho = 1.0 - (W - acov) / var_plus
        rho[0] = 1.0
        p0 = rho[0] + rho[1]
        tau = -1.0 + 2.0 * p0
        prev = p0.copy()
        running = np.ones(D, dtype=bool)                              # no non-positive pair met so far
        T = 1
        while 2 * T + 1 <= L:
            pt = rho[2 * T] + rho[2 * T + 1]
            running &= pt > 0.0
            pm = np.where(pt < prev, pt, prev)
            prev = np.where(running, pm, prev)
            tau = np.where(running, tau + 2.0 * pm, tau)
            T += 1
        ess = (md * nd) / tau
    return SimpleNamespace(mean=gm, sd=sd, within_var=W, rhat=rhat, ess=ess, ess_truncated=running.astype(np.uint64), autocorr=rho,
                           chain_mean=mean_m, chain_var=var_m, n_series=M, n_per_series=n)


FIELDS = ("mean", "sd", "within_var", "rhat", "ess", "ess_truncated", "autocorr", "chain_mean", "chain_var")


def ar1_draws():
    """the AR(1) input of the issue: 200 draws x 64 chains x 5 columns with lag-1 correlations 0, 0.3, 0.6, 0.9, -0.3"""
    rng = np.random.default_rng(7)
    N, C = 200, 64
    rhos = np.array([0.0, 0.3, 0.6, 0.9, -0.3])
    x = np.zeros((N, C, 5))
    x[0] = rng.normal(size=(C, 5))
    for t in range(1, N):
        x[t] = rhos * x[t - 1] + np.sqrt(1 - rhos**2) * rng.normal(size=(C, 5))
    return x, rhos


def check_ar1_bands(summarize_fn):
    """the statistical assertions of the issue on the AR(1) input, for any implementation of the definition"""
    x, rhos = ar1_draws()
    N, C = x.shape[:2]
    s = summarize_fn(x, True, 32)
    ratio = s.ess / (N * C * (1 - rhos) / (1 + rhos))
    print("ess ratios", ratio, "truncated", s.ess_truncated, "rhat", s.rhat)
    for j in (0, 1, 2, 4):
        assert 0.8 <= ratio[j] <= 1.35, (j, ratio[j])
    assert list(s.ess_truncated) == [0, 0, 0, 1, 0]
    assert (s.rhat[:3] < 1.02).all()
    shifted = x.copy()
    shifted[:, :8] += 1.0
    r = summarize_fn(shifted, True, 32).rhat
    print("shifted rhat", r)
    assert (r > 1.04).all()
    drift = x.copy()
    drift[N // 2:] += 0.5
    r_split, r_unsplit = summarize_fn(drift, True, 32).rhat, summarize_fn(drift, False, 32).rhat
    print("drift split", r_split, "unsplit", r_unsplit)
    assert (r_split > 1.02).all() and (r_unsplit[:3] < 1.01).all()
