"""nm_summarize_draws (posterior summaries on the device; defined by this repository, include/nuts_amd.h) without a GPU: the layout of
its two structures, the arguments it refuses before any device call, and the numpy restatement of its definition (tests/summary_ref.py)
against independent numpy and against AR(1) series whose effective sample size is known."""
import ctypes as C
import os

import numpy as np

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import summary_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")


def test_structure_sizes_and_abi_version():
    assert C.sizeof(_lib.NmSummarySpec) == 9 * 8 and C.sizeof(_lib.NmSummaryOutputs) == 12 * 8
    L = N.load_library()
    assert L.nm_abi_version() >= 18
    header = open(HEADER).read()
    assert int(header.split("#define NM_SUMMARY_CHUNK_CHAINS")[1].split()[0]) == N.NM_SUMMARY_CHUNK_CHAINS == 32
    assert "nm_summarize_draws" in _lib.ABI_SYMBOLS and hasattr(L, "nm_summarize_draws")


def _call(spec, draws=0x1000, outputs=True):
    """the status of a call whose arguments must be refused before anything touches the device (the pointer is never read)"""
    L = N.load_library()
    out = _lib.NmSummaryOutputs()
    return L.nm_summarize_draws(C.byref(spec) if spec is not None else None, C.c_void_p(draws or None),
                                C.byref(out) if outputs else None, None)


def _spec(n_draws=20, n_chains=4, dim=3, split=1, max_lag=8, ids=None):
    s = _lib.NmSummarySpec(n_draws, n_chains, dim, split, max_lag, 0, None)
    if ids is not None:
        s._keep = np.ascontiguousarray(ids, dtype=np.uint64)
        s.n_chain_ids, s.h_chain_ids = len(s._keep), s._keep.ctypes.data if len(s._keep) else 0x1000
    return s


def test_invalid_arguments_are_refused_without_a_device():
    assert _call(None) == 1
    assert _call(_spec(), draws=0) == 1
    assert _call(_spec(), outputs=False) == 1
    assert _call(_spec(dim=0)) == 1
    assert _call(_spec(n_chains=0)) == 1
    assert _call(_spec(n_draws=0)) == 1
    assert _call(_spec(max_lag=0)) == 1
    assert _call(_spec(max_lag=65)) == 1
    assert _call(_spec(n_draws=3, split=1)) == 1                  # n = 1
    assert _call(_spec(n_draws=1, split=0)) == 1                  # n = 1
    assert _call(_spec(n_chains=1, split=0)) == 1                 # M = 1
    assert _call(_spec(split=0, ids=[2])) == 1                    # M = 1 after the selection
    assert _call(_spec(ids=[])) == 1                              # M = 0
    assert _call(_spec(ids=[0, 2, 2])) == 1                       # not strictly increasing
    assert _call(_spec(ids=[2, 1])) == 1
    assert _call(_spec(ids=[0, 4])) == 1                          # out of range
    assert b"nm_summarize_draws" in N.load_library().nm_summary_last_error()


def test_restatement_against_independent_numpy():
    """mean, W and rhat computed the short way (np.mean, np.var(ddof=1)).  Error bound: a serial sum of up to 1000 non-negative terms
    carries a relative error of at most n * 2^-53 ~ 1e-13; widened tenfold."""
    rng = np.random.default_rng(11)
    for (n_draws, n_chains, dim), split in (((60, 37, 5), True), ((41, 6, 3), True), ((30, 70, 4), False)):
        x = rng.normal(size=(n_draws, n_chains, dim)) * np.exp(rng.uniform(-3, 3, size=dim)) + rng.normal(size=dim)
        s = summary_ref.summarize(x, split=split, max_lag=10)
        n = n_draws // 2 if split else n_draws
        ser = np.concatenate([x[:n], x[n_draws - n:]], axis=1) if split else x
        W = np.var(ser, axis=0, ddof=1).mean(axis=0)
        B_over_n = np.var(ser.mean(axis=0), axis=0, ddof=1)
        rhat = np.sqrt((W * (n - 1) / n + B_over_n) / W)
        assert s.n_series == ser.shape[1] and s.n_per_series == n
        assert np.allclose(s.within_var, W, rtol=1e-12, atol=0) and np.allclose(s.rhat, rhat, rtol=1e-12, atol=0)
        assert (np.abs(s.mean - ser.mean(axis=(0, 1))) <= 1e-12 * np.abs(x).max()).all()
        assert (np.abs(s.chain_mean - ser.mean(axis=0)) <= 1e-12 * np.abs(x).max()).all()
        assert np.allclose(s.chain_var, np.var(ser, axis=0, ddof=1), rtol=1e-12, atol=0)
        assert (s.autocorr[0] == 1.0).all() and s.autocorr.shape == (11, dim)


def test_restatement_on_ar1_series():
    """ESS / (N C (1 - rho) / (1 + rho)) in [0.8, 1.35], the truncation flag only on the rho = 0.9 column (32 lags are too few there), and
    R-hat's reaction to shifted chains and to a drift between the halves.  Bounds: a prototype of the definition on this seed gave ESS
    ratios 1.000, 1.090, 1.071, 1.169 (0.95 - 1.25 over five more seeds), shifted R-hat >= 1.050, split drift >= 1.029, unsplit <= 1.006."""
    summary_ref.check_ar1_bands(lambda x, split, lag: summary_ref.summarize(x, split=split, max_lag=lag))
