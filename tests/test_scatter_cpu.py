"""nm_pooled_scatter and the pooled low-rank estimate without a GPU: the header against the library, the arguments the call
refuses before any device call, the restatement of its definition (tests/scatter_ref.py) against an extended-precision scatter, and the
host half of the pooled low-rank adaptation — lowrank_from_moments against the oracle's compute_update and the reference's two known
answers, scatter_merge against the scatter of the concatenated rows."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib, pooled

import scatter_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")
KATS = json.load(open(os.path.join(HERE, "golden", "reference_kats.json")))["lowrank_estimator"]


def _define(name):
    return int(open(HEADER).read().split("#define " + name)[1].split()[0])


def test_header_against_library_and_package():
    L = N.load_library()
    assert _define("NM_ABI_VERSION") == 20 == L.nm_abi_version()
    assert _define("NM_SCATTER_SLAB_MIN_ROWS") == N.NM_SCATTER_SLAB_MIN_ROWS == _lib.NM_SCATTER_SLAB_MIN_ROWS
    assert _define("NM_SCATTER_MAX_SLABS") == N.NM_SCATTER_MAX_SLABS == _lib.NM_SCATTER_MAX_SLABS
    assert _define("NM_SCATTER_MAX_DIM") == N.NM_SCATTER_MAX_DIM == 1024
    assert "nm_pooled_scatter" in _lib.ABI_SYMBOLS and hasattr(L, "nm_pooled_scatter")
    assert callable(N.pooled_scatter) and callable(N.covariance_draws) and callable(pooled.pooled_lowrank_warmup)


def _call(n_rows=10, dim=3, rows=0x1000, center=0x1000, scatter=0x1000, stats=None, count=None):
    """the status of a call whose arguments must be refused before anything touches the device (the pointers are never read)"""
    return N.load_library().nm_pooled_scatter(n_rows, dim, C.c_void_p(rows or None), C.c_void_p(center or None), stats, C.c_void_p(scatter or None), count, None)


def test_invalid_arguments_are_refused_without_a_device():
    assert _call(rows=0) == 1
    assert _call(center=0) == 1
    assert _call(scatter=0) == 1
    assert _call(n_rows=0) == 1
    assert _call(dim=0) == 1
    assert _call(dim=N.NM_SCATTER_MAX_DIM + 1) == 1
    assert b"nm_pooled_scatter" in N.load_library().nm_pooled_last_error() and b"NM_SCATTER_MAX_DIM" in N.load_library().nm_pooled_last_error()
    import torch
    if not torch.cuda.is_available():        # everything else is accepted and then fails for want of a device: there is no CPU fallback
        assert _call(dim=N.NM_SCATTER_MAX_DIM) == 2


def test_slabs_are_cut_by_the_row_count_alone():
    assert scatter_ref.slabs(1) == (1, 4) and scatter_ref.slabs(256) == (1, 256) and scatter_ref.slabs(257) == (2, 132)
    assert scatter_ref.slabs(256 * 64) == (64, 256) and scatter_ref.slabs(256 * 64 + 1) == (64, 260) and scatter_ref.slabs(10**6) == (64, 15628)
    # With the constants 256 and 64 NO row count leaves the trailing slab empty.  An empty one needs (k - 1) R >= n with k slabs; R < n / k + 4, so
    # n < 4 k (k - 1); below the clamp k = ceil(n / 256) gives n > 256 (k - 1), hence k > 64; at the clamp k = 64 and n > 16128 > 4 * 64 * 63 = 16128.
    # The kernel still serves such a slab (it adds +0.0), should the constants be retuned: this pins the fact for the constants as they are.
    if (N.NM_SCATTER_SLAB_MIN_ROWS, N.NM_SCATTER_MAX_SLABS) == (256, 64):
        for n in range(1, 70000):
            k, R = scatter_ref.slabs(n)
            assert (k - 1) * R < n <= k * R and R % 4 == 0, n


def generic(rng, n, dim):
    """generic doubles: per-column scales e^(+-3), offsets +-10"""
    return rng.normal(size=(n, dim)) * np.exp(rng.uniform(-3, 3, size=dim)) + rng.normal(size=dim) * 10.0


@pytest.mark.parametrize("n,dim", [(1, 1), (5, 16), (200, 8), (257, 17), (1000, 33), (16500, 4)])
def test_restatement_against_extended_precision(n, dim):
    """|S - exact| <= (n + 4) 2^-53 sum_r |y_ri y_rj| per entry — derived (scatter_ref.scatter_bound): one rounding per y, one per fma step."""
    rng = np.random.default_rng(n * 100 + dim)
    x = generic(rng, n, dim)
    for center in (np.zeros(dim), x.mean(axis=0)):
        S, count = scatter_ref.scatter(x, center)
        exact, bound = scatter_ref.scatter_bound(x, center)
        assert count == n and (S == S.T).all()
        assert (np.abs(S.astype(np.longdouble) - exact) <= bound).all(), float((np.abs(S - exact) / np.maximum(bound, 1e-300)).max())
    st = scatter_ref.stats_rows(n, rng)
    keep = scatter_ref.kept(st, n)
    x[~keep] = np.nan                                    # a row that is left out is selected away, never multiplied by zero
    S, count = scatter_ref.scatter(x, np.zeros(dim), st)
    exact, bound = scatter_ref.scatter_bound(x, np.zeros(dim), keep)
    assert count == keep.sum() and (np.abs(S.astype(np.longdouble) - exact) <= bound).all()


def test_row_rule_is_the_collectors():
    st = np.zeros(8, dtype=N.STATS_DTYPE)
    st["index_in_trajectory"] = [0, 1, -1, 4, -5, 5, 3, 2]
    st["diverging"] = [0, 0, 0, 1, 1, 1, 0, 0]
    st["chain_status"] = [0, 0, 0, 0, 0, 0, 1, 0]
    assert scatter_ref.kept(st, 8).tolist() == [False, True, True, False, True, True, False, True]
    assert not scatter_ref.kept(np.zeros(3, dtype=N.STATS_DTYPE), 3).any()          # an unwritten, zero-filled row


# ---- lowrank_from_moments ------------------------------------------------------------------------------------------------------------

def window(rng, dim, n, rank=3):
    """draws of a correlated normal and their gradients, [n][dim]"""
    u = np.linalg.qr(rng.normal(size=(dim, min(rank, dim))))[0]
    sigma = np.eye(dim) + u @ np.diag(rng.uniform(5.0, 50.0, u.shape[1])) @ u.T
    sc = np.exp(rng.normal(0, 0.5, dim))
    sigma = np.diag(sc) @ sigma @ np.diag(sc)
    m = rng.normal(size=dim)
    x = rng.multivariate_normal(m, sigma, size=n)
    return x, -(x - m) @ np.linalg.inv(sigma)


def moments(x):
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    y = x - mean
    return float(n), mean, y.T @ y


def operator(vals, vecs):
    """what the transformation uses of the eigenpairs: U (lambda - 1) U' (vecs [n_eig][dim])"""
    return (vecs.T * (vals - 1.0)) @ vecs


# The largest differences between the two routes measured when the estimate was written (dim 8 x 200 rows, 32 x 4000, 16 x 17, 3 x 20):
# stds 2e-16 relative, eigenvalues 3e-12 relative, the low-rank operator 1e-11, mu_low_rank 4e-11 — times 100, because the two routes
# decompose different matrices (the window's thin SVDs and a pivoted QR against the D x D moments) and agree up to rounding that the
# decompositions amplify, not bit for bit.  The operator and mu are compared relative to their own size (1 where that is smaller).
TOL_STDS, TOL_VALS, TOL_OP, TOL_MU = 2e-14, 3e-10, 1e-9, 4e-9


def eigh_ld(a):
    """eigenvalues and eigenvectors of a symmetric matrix in np.longdouble: cyclic Jacobi rotations (numpy's eigh stops at binary64)"""
    a = np.array(a, dtype=np.longdouble)
    n = a.shape[0]
    v = np.eye(n, dtype=np.longdouble)
    eps = np.finfo(np.longdouble).eps
    for _ in range(60):
        off = np.sqrt(((a - np.diag(np.diag(a))) ** 2).sum())
        if off <= eps * np.sqrt((np.diag(a) ** 2).sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if a[p, q] == 0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = (1 if theta >= 0 else -1) / (abs(theta) + np.hypot(theta, np.longdouble(1)))
                c = 1 / np.sqrt(t * t + 1)
                sn = t * c
                for m, axis in ((a, 1), (a, 0), (v, 1)):          # columns of a, rows of a, columns of v
                    mp, mq = (m[:, p].copy(), m[:, q].copy()) if axis else (m[p, :].copy(), m[q, :].copy())
                    if axis:
                        m[:, p], m[:, q] = c * mp - sn * mq, sn * mp + c * mq
                    else:
                        m[p, :], m[q, :] = c * mp - sn * mq, sn * mp + c * mq
    return np.diag(a).copy(), v


def spectrum_ld(x, g, gamma):
    """the eigenvalues of the estimate's geometric mean (every pair, before the cutoff) from the window in np.longdouble — the formulas
    of lowrank_from_moments with 64 instead of 53 bits — and kappa = max(cond A, cond B) of the two matrices whose mean it is"""
    x, g = x.astype(np.longdouble), g.astype(np.longdouble)
    n, dim = x.shape
    yx, yg = x - x.sum(axis=0) / n, g - g.sum(axis=0) / n
    sx, sg = yx.T @ yx, yg.T @ yg
    sigma = np.sqrt(np.sqrt(np.diag(sx) / np.diag(sg)))
    a = sx / np.outer(sigma, sigma) / gamma + np.eye(dim)
    b = sg * np.outer(sigma, sigma) / gamma + np.eye(dim)
    w, u = eigh_ld(b)
    g_sqrt, g_inv_sqrt = (u * np.sqrt(w)) @ u.T, (u / np.sqrt(w)) @ u.T
    mw, mu = eigh_ld(g_sqrt @ a @ g_sqrt)
    vals = eigh_ld(g_inv_sqrt @ ((mu * np.sqrt(mw)) @ mu.T) @ g_inv_sqrt)[0]
    wa = eigh_ld(a)[0]
    return np.sort(vals).astype(np.float64), float(max(wa.max() / wa.min(), w.max() / w.min()))


def test_longdouble_eigh_is_an_eigendecomposition():
    rng = np.random.default_rng(0)
    m = rng.normal(size=(9, 9))
    m = m @ m.T + np.diag(np.exp(rng.uniform(-8, 8, 9)))
    w, v = eigh_ld(m)
    ml = m.astype(np.longdouble)
    assert float(np.abs(v @ np.diag(w) @ v.T - ml).max()) <= 64 * 2.0**-64 * np.abs(m).max()
    assert float(np.abs(v.T @ v - np.eye(9)).max()) <= 64 * 2.0**-64
    assert np.abs(np.sort(w).astype(np.float64) / np.linalg.eigvalsh(m) - 1).max() <= 9 * 2.0**-53 * np.linalg.cond(m)


# Both routes lose accuracy in proportion to the conditioning of the window, and a window of n = dim + 1 rows has a sample covariance of ANY
# conditioning.  The bound: the estimate is three symmetric eigendecompositions and seven dim x dim products, each backward stable with an
# error of at most about dim 2^-53 relative to its operands; the inverse square root of B and the congruences with it amplify an error by
# at most kappa = max(cond A, cond B), the two matrices whose geometric mean is taken.  Ten such steps: 10 dim kappa 2^-53 per route,
# against the same formulas in np.longdouble (whose own error is 2^-11 of that).  Asserted on the FIRST window of each stream, whatever
# its conditioning (the first 16 x 17 window has cond S_x 3.3e5).
def kappa_bound(dim, kappa):
    return 10 * dim * kappa * 2.0**-53


@pytest.mark.parametrize("dim,n", [(8, 200), (32, 4000), (16, 17), (3, 20)])
def test_both_routes_against_extended_precision_on_an_unselected_window(dim, n):
    from oracle import lowrank as LR
    x, g = window(np.random.default_rng(dim * 7 + n), dim, n)
    exact, kappa = spectrum_ld(x, g, 1e-5)
    cx, mx, sx = moments(x)
    _, mg, sg = moments(g)
    mine = np.sort(pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 1.0)[2])          # cutoff 1: every pair
    theirs = np.sort(LR.compute_update(x.T, g.T, 1e-5, 1.0)[2])
    bound = kappa_bound(dim, kappa)
    print(f"dim {dim} x {n} rows: kappa {kappa:.3g}, bound {bound:.3g}, moments route {np.abs(mine / exact - 1).max():.3g}, "
          f"oracle {np.abs(theirs / exact - 1).max():.3g}, between them {np.abs(mine / theirs - 1).max():.3g}")
    assert len(mine) == len(theirs) == dim and bound < 1e-3
    assert np.abs(mine / exact - 1).max() <= bound
    assert np.abs(theirs / exact - 1).max() <= bound


# The fixed tolerances above were measured on windows of moderate conditioning; where the bound just derived allows more than they do, no
# route can be held to them.  They are asserted on the first window of each stream whose cond(S_x) is at most 3e4 — a property of the DATA
# alone, and the second window of the 16 x 17 stream; the unselected first windows are the test above.
KAPPA_MAX = 3e4


@pytest.mark.parametrize("dim,n", [(8, 200), (32, 4000), (16, 17), (3, 20)])
def test_moments_route_against_the_oracles_compute_update(dim, n):
    from oracle import lowrank as LR
    rng = np.random.default_rng(dim * 7 + n)
    while True:
        x, g = window(rng, dim, n)
        if np.linalg.cond(moments(x)[2]) <= KAPPA_MAX:
            break
    cx, mx, sx = moments(x)
    _, mg, sg = moments(g)
    kept = []
    for cutoff in (2.0, 1.0):          # the reference's filter, and every pair (the 3 x 20 window keeps none under the filter)
        want = LR.compute_update(x.T, g.T, 1e-5, cutoff)
        got = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, cutoff)
        assert want is not None and got is not None
        stds, mean, vals, vecs, mu = got
        w_stds, w_mean, w_vals, w_vecs, w_mu = want
        assert len(vals) == len(w_vals) and vecs.shape == (len(vals), dim)          # the number of kept eigenvalues agrees
        assert np.abs(stds / w_stds - 1).max() <= TOL_STDS and np.abs(mean - w_mean).max() <= TOL_STDS * 100 * np.abs(w_mean).max()
        if len(vals):
            assert np.abs(np.sort(vals) / np.sort(w_vals) - 1).max() <= TOL_VALS
            assert np.abs(vecs @ vecs.T - np.eye(len(vals))).max() < 1e-12
        op, w_op = operator(vals, vecs), operator(w_vals, w_vecs.T)
        assert np.abs(op - w_op).max() <= TOL_OP * max(1.0, np.abs(w_op).max())
        assert np.abs(mu - w_mu).max() <= TOL_MU * max(1.0, np.abs(w_mu).max())
        kept.append(len(vals))
    assert kept[1] == dim and np.abs(op).max() > 0 and np.abs(mu).max() > 0          # (the cutoff-1 pass compares something in every shape)


def test_whitened_target_has_condition_number_below_cutoff_squared():
    """For a normal target g is linear in x, C_g = P C_x P for ANY sample: the estimate is exact up to the eigenvalues the cutoff leaves."""
    rng = np.random.default_rng(5)
    dim = 32
    x, g = window(rng, dim, 4000, rank=4)
    cx, mx, sx = moments(x)
    _, mg, sg = moments(g)
    sigma_true = np.linalg.inv(-np.linalg.lstsq(x - mx, g - mg, rcond=None)[0])
    for multiple in (1, 8):
        stds, mean, vals, vecs, mu = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=multiple)
        f_inv = (np.eye(dim) + (vecs.T * (vals**-0.5 - 1.0)) @ vecs) / stds          # z = F^-1 (x - mean): cov_z = F^-1 Sigma F^-T
        ev = np.linalg.eigvalsh(f_inv @ sigma_true @ f_inv.T)
        assert ev.max() / ev.min() <= 4.0 * 1.05, (multiple, ev.max() / ev.min())
    d = np.sqrt(np.diag(sigma_true))
    ev = np.linalg.eigvalsh(sigma_true / np.outer(d, d))
    assert ev.max() / ev.min() > 20.0                                                  # what a diagonal scaling leaves


def test_reference_known_answers():
    k = KATS["spd_mean"]                                   # adapt/low_rank.rs:354-381: diag(1, 4, 8), diag(1, 1, 0.5) -> diag(1, 2, 4)
    got = pooled._spd_mean(np.diag(k["x_diag"]), np.diag(k["y_diag"]))
    assert np.allclose(got, np.diag(k["expected_diag"]), rtol=k["rel_tol"], atol=k["abs_tol"])
    k = KATS["estimate_mass_matrix"]                       # :383-407: grads = -draws gives eigenvalues 1, so nothing is kept
    rng = np.random.default_rng(1)
    x = rng.normal(size=tuple(k["shape"]))
    cx, mx, sx = moments(x)
    _, mg, sg = moments(-x)
    stds, mean, vals, vecs, mu = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, k["gamma"], 2.0)
    assert len(vals) == 0 and vecs.shape == (0, 3) and np.allclose(stds, 1.0, rtol=1e-14) and np.abs(mean).max() < 1e-14
    # the eigenvalues themselves, before the filter: a cutoff of 1 + tol keeps none either
    assert len(pooled.lowrank_from_moments(cx, mx, sx, mg, sg, k["gamma"], 1.0 + k["rel_tol"] + k["abs_tol"])[2]) == 0


def test_no_estimate_from_too_few_or_non_finite_moments():
    rng = np.random.default_rng(2)
    x, g = window(rng, 4, 50)
    cx, mx, sx = moments(x)
    _, mg, sg = moments(g)
    assert pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0) is not None
    assert pooled.lowrank_from_moments(2.0, mx, sx, mg, sg, 1e-5, 2.0) is None
    assert pooled.lowrank_from_moments(float("nan"), mx, sx, mg, sg, 1e-5, 2.0) is None
    for pos in range(4):
        for bad in (np.nan, np.inf):
            args = [mx.copy(), sx.copy(), mg.copy(), sg.copy()]
            args[pos].flat[1] = bad
            assert pooled.lowrank_from_moments(cx, *args, 1e-5, 2.0) is None
    assert pooled.lowrank_from_moments(cx, mx, sx, mg, np.zeros_like(sg), 1e-5, 2.0) is None       # a gradient that does not vary: sigma = inf
    assert pooled.lowrank_from_moments(cx, mx, np.zeros_like(sx), mg, sg, 1e-5, 2.0) is None


def test_rank_multiple_keeps_the_next_pairs_with_their_own_eigenvalues():
    rng = np.random.default_rng(9)
    dim = 24
    x, g = window(rng, dim, 3000, rank=3)
    cx, mx, sx = moments(x)
    _, mg, sg = moments(g)
    s1, m1, v1, u1, mu1 = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0)
    m = next(k for k in (8, 7, 5) if len(v1) % k)                                        # a multiple the kept set is not one of already
    want = min(dim, m * -(-len(v1) // m))
    s8, m8, v8, u8, mu8 = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=m)
    sa, ma, va, ua, _ = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 1.0)       # cutoff 1 keeps every pair
    assert 0 < len(v1) < want and len(v8) == want and u8.shape == (want, dim) and len(va) == dim
    assert (s1 == s8).all() and (m1 == m8).all()
    assert set(v1.tolist()) <= set(v8.tolist())
    extra = sorted(set(v8.tolist()) - set(v1.tolist()))
    assert len(extra) == want - len(v1) and all(0.5 <= e <= 2.0 and e != 1.0 for e in extra)   # their own lambda, inside the cutoff
    rest = sorted(set(va.tolist()) - set(v1.tolist()), key=lambda e: -abs(np.log(e)))
    assert sorted(extra) == sorted(rest[:len(extra)])                                       # the next ones in order of |ln lambda|
    assert len(pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=8)[2]) % 8 == 0
    # a strictly closer approximation of the full operator than dropping them
    full = operator(va, ua)
    assert np.linalg.norm(operator(v8, u8) - full) < np.linalg.norm(operator(v1, u1) - full)
    # max_rank (an engine's lowrank_max_rank): the largest multiple that fits, the pairs of largest |ln lambda|
    by_size = sorted(v8.tolist(), key=lambda e: -abs(np.log(e)))
    for cap, m_, n_want in ((want - 1, m, want - m), (want, m, want), (dim, m, want), (3, 1, 3), (m - 1, m, m - 1)):
        vc, uc = pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=m_, max_rank=cap)[2:4]
        pool = by_size if m_ == m else sorted(v1.tolist(), key=lambda e: -abs(np.log(e)))
        assert len(vc) == n_want and uc.shape == (n_want, dim) and sorted(vc.tolist()) == sorted(pool[:n_want]), (cap, m_)
    # capped at dim; a kept set that already is a multiple stays
    assert len(pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=dim + 5)[2]) == dim
    assert len(pooled.lowrank_from_moments(cx, mx, sx, mg, sg, 1e-5, 2.0, rank_multiple=len(v1))[2]) == len(v1)


def test_scatter_merge_against_the_concatenated_rows():
    """Chan's merge against the scatter of the concatenated rows about their mean, within the derived bound of the scatter itself:
    (n + 4) 2^-53 sum_r |y_ri y_rj| (scatter_ref.scatter_bound)."""
    rng = np.random.default_rng(4)
    for (na, nb, dim) in ((100, 37, 5), (1, 300, 3), (50, 50, 12)):
        x = generic(rng, na + nb, dim)
        a, b = x[:na], x[na:]
        ta = (float(na), a.mean(axis=0), scatter_ref.scatter(a, a.mean(axis=0))[0])
        tb = (float(nb), b.mean(axis=0), scatter_ref.scatter(b, b.mean(axis=0))[0])
        n, mean, S = pooled.scatter_merge(ta, tb)
        exact_mean = x.astype(np.longdouble).sum(axis=0) / (na + nb)
        y = x.astype(np.longdouble) - exact_mean
        exact, mag = y.T @ y, np.abs(y).T @ np.abs(y)
        assert n == na + nb and np.abs(mean - exact_mean).max() <= 8 * 2.0**-53 * np.abs(x).max()
        assert (np.abs(S - exact) <= (na + nb + 4) * 2.0**-53 * mag).all()
    empty = (0.0, np.zeros(3), np.zeros((3, 3)))
    t = (4.0, np.ones(3), np.eye(3))
    for got in (pooled.scatter_merge(empty, t), pooled.scatter_merge(t, empty)):
        assert got[0] == 4.0 and (got[1] == t[1]).all() and (got[2] == t[2]).all()


def test_window_schedule_is_pooled_warmups():
    """the schedule both pooled drivers share, restated: 10-draw windows in the first 30 %, then 80 growing by 1.5x, none in the last 15 %"""
    assert pooled.window_schedule(300) == [10] * 9 + [80]
    assert pooled.window_schedule(1000) == [10] * 30 + [80, 120, 180]
    assert pooled.window_schedule(20) == []
