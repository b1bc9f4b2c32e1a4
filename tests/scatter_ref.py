"""The definition of nm_pooled_scatter (include/nuts_amd.h) restated on the host — a helper, not a test.

The slabs and the row rule are restated here in Python from the header's text (the two slab constants are read from the package); the
fma chains themselves run in a few lines of C++ (tests/cpp/scatter_ref.cpp: std::fma, -ffp-contract=off) because numpy has no fused
multiply-add.  One fma per kept row and output in row order from +0.0 per slab, the slab values added in slab order from +0.0: the
device result can be compared bit for bit.  n_rows * dim^2 of a case should stay below about 5e7."""
import ctypes as C
import os
import subprocess

import numpy as np

from nuts_rs_amd import NM_SCATTER_MAX_SLABS, NM_SCATTER_SLAB_MIN_ROWS, STATS_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "scatter_ref.cpp")
LIB = os.path.join(HERE, "cpp", "libscatter_ref.so")
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        _lib.scatter_ref.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        _lib.scatter_ref.restype = None
    return _lib


def slabs(n_rows):
    """(n_slabs, R): slab s is rows [s R, min((s + 1) R, n_rows))"""
    n_slabs = min(max(-(-n_rows // NM_SCATTER_SLAB_MIN_ROWS), 1), NM_SCATTER_MAX_SLABS)
    per = -(-n_rows // n_slabs)
    return n_slabs, 4 * (-(-per // 4))


def kept(stats, n_rows):
    """which rows count (nm_pooled_partials' rule): the chain is healthy and the draw is one the reference's collector keeps"""
    if stats is None:
        return np.ones(n_rows, dtype=bool)
    st = np.asarray(stats).reshape(-1)
    idx = st["index_in_trajectory"].astype(np.int64)
    good = np.where(st["diverging"] != 0, np.abs(idx) > 4, idx != 0)
    return (st["chain_status"] == 0) & good


def scatter(rows, center, stats=None):
    """(S [dim][dim], count) as nm_pooled_scatter defines them"""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    dim = x.shape[-1]
    x = x.reshape(-1, dim)
    c = np.ascontiguousarray(center, dtype=np.float64)
    n_rows = x.shape[0]
    keep = np.ascontiguousarray(kept(stats, n_rows), dtype=np.uint8)
    n_slabs, R = slabs(n_rows)
    S = np.empty((dim, dim))
    _load().scatter_ref(n_rows, dim, x.ctypes.data, c.ctypes.data, None if stats is None else keep.ctypes.data, R, n_slabs, S.ctypes.data)
    return S, float(keep.sum())


def scatter_bound(rows, center, keep=None):
    """(exact scatter in extended precision, the derived bound per entry) for the restatement against np.longdouble: one rounding per y
    (relative 2^-53 each, two factors) and one per fma step and slab addition, at most n + 4 roundings of relative size 2^-53 on partial
    sums bounded by sum_r |y_ri y_rj|:  (n + 4) 2^-53 sum_r |y_ri y_rj|."""
    x = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1])
    if keep is not None:
        x = x[np.asarray(keep, dtype=bool)]
    y = x.astype(np.longdouble) - np.asarray(center, dtype=np.float64).astype(np.longdouble)
    exact = y.T @ y
    bound = (x.shape[0] + 4) * 2.0**-53 * (np.abs(y).T @ np.abs(y))
    return exact, bound


def stats_rows(n_rows, rng, leave_out=0.3):
    """a statistics buffer that leaves rows out in every way the rule knows: stopped chains, the first point of a trajectory, divergent
    draws near their start — and keeps divergent draws far from it"""
    st = np.zeros(n_rows, dtype=STATS_DTYPE)
    st["index_in_trajectory"] = rng.integers(1, 30, n_rows) * rng.choice([-1, 1], n_rows)
    u = rng.uniform(size=n_rows)
    st["chain_status"][u < leave_out / 3] = 2
    st["index_in_trajectory"][(u >= leave_out / 3) & (u < 2 * leave_out / 3)] = 0
    div = (u >= 2 * leave_out / 3) & (u < leave_out)
    st["diverging"][div] = 1
    st["index_in_trajectory"][div] = rng.integers(-6, 7, int(div.sum()))
    return st
