"""nm_quantile_draws (posterior quantiles on the device; defined by this repository, include/nuts_amd.h) without a GPU: the layout of
its two structures, the arguments it refuses before any device call, and the numpy restatement of its definition (tests/quantile_ref.py)
against np.quantile and, column by column, against values worked out by hand."""
import ctypes as C
import os

import numpy as np

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import quantile_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")


def test_structure_sizes_symbol_and_constant():
    assert C.sizeof(_lib.NmQuantileSpec) == 9 * 8 and C.sizeof(_lib.NmQuantileOutputs) == 4 * 8
    L = N.load_library()
    assert L.nm_abi_version() >= 19
    header = open(HEADER).read()
    assert int(header.split("#define NM_QUANTILE_MAX_PROBS")[1].split()[0]) == N.NM_QUANTILE_MAX_PROBS == 16
    for name in ("nm_quantile_draws", "nm_quantile_last_error"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert callable(N.quantile_draws)


def _spec(n_draws=20, n_chains=4, dim=3, probs=(0.5,), ids=None, null_probs=False):
    s = _lib.NmQuantileSpec(n_draws, n_chains, dim, len(probs), None, 0, None)
    s._p = np.ascontiguousarray(probs, dtype=np.float64)
    s.h_probs = None if null_probs else (s._p.ctypes.data if len(s._p) else 0x1000)
    if ids is not None:
        s._keep = np.ascontiguousarray(ids, dtype=np.uint64)
        s.n_chain_ids, s.h_chain_ids = len(s._keep), s._keep.ctypes.data if len(s._keep) else 0x1000
    return s


def _call(spec, draws=0x1000, outputs=(0x1000, 0x1000)):
    """the status of a call whose arguments must be refused before anything touches the device (the pointers are never read)"""
    L = N.load_library()
    out = None if outputs is None else _lib.NmQuantileOutputs(outputs[0] or None, outputs[1] or None)
    return L.nm_quantile_draws(C.byref(spec) if spec is not None else None, C.c_void_p(draws or None),
                               C.byref(out) if out is not None else None, None)


def test_invalid_arguments_are_refused_without_a_device():
    assert _call(None) == 1
    assert _call(_spec(), draws=0) == 1
    assert _call(_spec(), outputs=None) == 1
    assert _call(_spec(), outputs=(0, 0)) == 1                   # both outputs absent
    assert _call(_spec(null_probs=True)) == 1
    assert _call(_spec(dim=0)) == 1
    assert _call(_spec(n_chains=0)) == 1
    assert _call(_spec(n_draws=0)) == 1
    assert _call(_spec(probs=())) == 1
    assert _call(_spec(probs=[0.5] * 17)) == 1
    assert _call(_spec(probs=[0.5, np.nan])) == 1
    assert _call(_spec(probs=[-1e-300])) == 1
    assert _call(_spec(probs=[0.1, np.nextafter(1.0, 2.0)])) == 1
    assert _call(_spec(probs=[np.inf])) == 1
    assert _call(_spec(ids=[])) == 1                             # empty
    assert _call(_spec(ids=[0, 2, 2])) == 1                      # not strictly increasing
    assert _call(_spec(ids=[2, 1])) == 1
    assert _call(_spec(ids=[0, 4])) == 1                         # out of range
    assert _call(_spec(n_draws=2**16, n_chains=2**16)) == 1      # n = 2^32: the counts are 32-bit
    assert _call(_spec(n_draws=2**31, n_chains=4, ids=[1, 3])) == 1
    assert _call(_spec(n_draws=1, n_chains=1, dim=2**31)) == 1   # the launch grid
    assert b"nm_quantile_draws" in N.load_library().nm_quantile_last_error()


def test_restatement_against_numpy_quantile():
    """Generic finite data against np.quantile(method="linear").  Bound 16 * 2^-53 * max|x| of the column — derived, not measured: each
    side does at most three roundings on operands bounded by 2 max|x|, at most 5 units of 2^-53 max|x| each side (one of 2, one of 2,
    one of 1), summed and rounded up to a power of two."""
    rng = np.random.default_rng(3)
    probs = [0.05, 0.5, 0.95, 0.0, 1.0, 0.25, 1.0 / 3.0, 0.999]
    for shape in ((60, 37, 5), (41, 6, 3), (1, 1, 2), (2, 1, 4), (17, 70, 10)):
        x = rng.normal(size=shape) * np.exp(rng.uniform(-3, 3, size=shape[2])) + rng.normal(size=shape[2]) * 10.0
        q, nan = quantile_ref.quantile(x, probs)
        want = np.quantile(x.reshape(-1, shape[2]), probs, axis=0, method="linear")
        bound = 16.0 * 2.0**-53 * np.abs(x).max(axis=(0, 1))
        assert q.shape == want.shape == (len(probs), shape[2]) and (nan == 0).all() and nan.dtype == np.uint64
        assert (np.abs(q - want) <= bound).all(), np.abs(q - want).max()
    ids = np.arange(0, 37, 3)
    x = rng.normal(size=(20, 37, 4))
    q, _ = quantile_ref.quantile(x, probs, chain_ids=ids)
    want = np.quantile(x[:, ids].reshape(-1, 4), probs, axis=0, method="linear")
    assert (np.abs(q - want) <= 16.0 * 2.0**-53 * np.abs(x).max(axis=(0, 1))).all()


def _col(values, probs):
    """the quantiles of one column given as a list"""
    q, nan = quantile_ref.quantile(np.asarray(values, dtype=np.float64).reshape(-1, 1, 1), probs)
    return q[:, 0], int(nan[0])


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def test_key_order_and_round_trip():
    tiny = 5e-324
    xs = np.array([-np.inf, -1.5, -2.5e-308, -tiny, -0.0, 0.0, tiny, 2.5e-308, 1.5, np.inf])
    k = quantile_ref.keys(xs)
    assert (np.diff(k.astype(object)) > 0).all()                          # strictly ascending as unsigned integers
    assert _bits(quantile_ref.unkeys(k)) == _bits(xs)


def test_special_columns_by_hand():
    # all-equal
    q, nan = _col([2.5] * 7, [0.0, 0.3, 0.5, 1.0])
    assert _bits(q) == _bits([2.5] * 4) and nan == 0
    # -0.0 and +0.0 mixed: sorted by key it is (-0, -0, +0, +0, +0); n - 1 = 4
    zeros = [0.0, -0.0, 0.0, -0.0, 0.0]
    q, _ = _col(zeros, [0.0, 0.25, 0.3, 0.5, 1.0])
    # p = 0.3: h = 1.2, x_(1) = -0, x_(2) = +0, keys differ: -0 + g * (+0 - -0) = -0 + 0 = +0
    assert _bits(q) == _bits([-0.0, -0.0, 0.0, 0.0, 0.0])
    q, _ = _col(zeros, [0.125])                                            # h = 0.5 between two -0.0: equal keys, x_(lo) itself
    assert _bits(q) == _bits([-0.0])
    # +-inf: (-inf, 1, 2, +inf), n - 1 = 3
    q, _ = _col([2.0, np.inf, -np.inf, 1.0], [0.0, 1.0, 0.5, 1.0 / 3.0, 0.1, 0.9])
    assert q[0] == -np.inf and q[1] == np.inf and q[2] == 1.5 and q[3] == 1.0
    assert np.isnan(q[4]) and q[5] == np.inf                               # -inf + 0.3 * (1 - -inf) = -inf + inf;  2 + 0.7 * (inf - 2)
    # an interval between -inf and +inf: inf - -inf = inf, g * inf = inf, -inf + inf = NaN — what IEEE gives
    q, nan = _col([-np.inf, np.inf], [0.5, 0.0, 1.0])
    assert np.isnan(q[0]) and q[1] == -np.inf and q[2] == np.inf and nan == 0
    # subnormals of both signs: (-3t, -t, t, 2t), exact arithmetic in the subnormal range
    t = 5e-324
    q, _ = _col([t, -t, 2 * t, -3 * t], [0.0, 0.5, 1.0, 1.0 / 3.0, 2.0 / 3.0])
    assert _bits(q[:3]) == _bits([-3 * t, -t + 0.5 * (t - -t), 2 * t]) and q[1] == 0.0
    assert q[3] == -t and q[4] == t
    # one NaN: every probability gives NaN, the count is exact
    q, nan = _col([1.0, np.nan, 3.0], [0.0, 0.5, 1.0])
    assert np.isnan(q).all() and nan == 1
    q, nan = _col([-np.nan, np.nan, 3.0], [0.5])                           # a NaN with its sign bit set counts as well
    assert np.isnan(q).all() and nan == 2
    # n = 1: every p gives the value
    q, _ = _col([-7.25], [0.0, 0.37, 1.0])
    assert _bits(q) == _bits([-7.25] * 3)
    # p of 0 and 1 are the extremes; a p whose h is an integer takes x_(lo) without arithmetic: n - 1 = 4, p = 0.75 -> h = 3
    q, _ = _col([5.0, 1.0, 4.0, 2.0, 3.0], [0.0, 1.0, 0.75, 0.25, 0.5])
    assert _bits(q) == _bits([1.0, 5.0, 4.0, 2.0, 3.0])
    assert quantile_ref.ranks(0.75, 5) == (3, 4, 0.0) and quantile_ref.ranks(1.0, 5) == (4, 4, 0.0)
    # an interior p: n - 1 = 3, p = 0.4 -> h = 1.2000000000000002 in binary64
    lo, hi, g = quantile_ref.ranks(0.4, 4)
    assert (lo, hi) == (1, 2) and g == 0.4 * 3.0 - 1.0
    q, _ = _col([10.0, 20.0, 40.0, 80.0], [0.4])
    assert q[0] == 20.0 + g * (40.0 - 20.0)
