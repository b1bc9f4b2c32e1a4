"""nm_transform_draws (rank transforms on the device; defined by this repository, include/nuts_amd.h) without a GPU: the
layout of its two structures, the arguments it refuses before any device call, the host twin of the normal score against mpmath, the
numpy restatement of the ranks (tests/rank_ref.py) against scipy and against values worked out by hand, and the statistical point of
the rank-normalised diagnostics on the restatement alone."""
import ctypes as C
import os
import re

import numpy as np

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import rank_ref
import summary_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "nuts_amd.h")
DRAWS, OUT, RANKS, COUNTS, PARAM = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000          # never read: far apart, so nothing overlaps


def test_structure_sizes_symbols_and_constants():
    assert C.sizeof(_lib.NmTransformSpec) == 10 * 8 and C.sizeof(_lib.NmTransformOutputs) == 5 * 8
    header = open(HEADER).read()
    for cname, mirror, words in (("nm_transform_spec", _lib.NmTransformSpec, 10), ("nm_transform_outputs", _lib.NmTransformOutputs, 5)):
        body = header.split("typedef struct " + cname + " {")[1].split("} " + cname)[0]
        fields = re.findall(r"(\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body))                                 # every field is one 8-byte word, or an array of them
        assert [n for n, _ in fields] == [n for n, _ in mirror._fields_], cname
        assert sum(int(k or 1) for _, k in fields) == words
    L = N.load_library()
    assert L.nm_abi_version() == 20 and int(header.split("#define NM_ABI_VERSION")[1].split()[0]) == 20          # purely additive
    slab = int(header.split("#define NM_RANK_SLAB_KEYS")[1].split()[0])
    assert slab == N.NM_RANK_SLAB_KEYS and slab <= 16384 and slab % 256 == 0
    for i, name in enumerate(("NM_TRANSFORM_RANK_NORMAL", "NM_TRANSFORM_FOLDED_RANK_NORMAL", "NM_TRANSFORM_INDICATOR_LE")):
        assert int(header.split("#define " + name)[1].split()[0]) == getattr(N, name) == i
    for name in ("nm_transform_draws", "nm_transform_last_error", "nm_rank_normal_score"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert callable(N.transform_draws) and callable(N.rank_diagnostics)


def _spec(n_draws=20, n_chains=4, dim=3, kind=0, split=1, ids=None):
    s = _lib.NmTransformSpec(n_draws, n_chains, dim, kind, split, 0, None, 0)
    if ids is not None:
        s._keep = np.ascontiguousarray(ids, dtype=np.uint64)
        s.n_chain_ids, s.h_chain_ids = len(s._keep), s._keep.ctypes.data if len(s._keep) else 0x1000
    return s


def _call(spec, draws=DRAWS, param=PARAM, outputs=(OUT, RANKS, COUNTS)):
    """the status of a call whose arguments must be refused before anything touches the device (the pointers are never read)"""
    L = N.load_library()
    out = None if outputs is None else _lib.NmTransformOutputs(outputs[0] or None, outputs[1] or None, outputs[2] or None)
    return L.nm_transform_draws(C.byref(spec) if spec is not None else None, C.c_void_p(draws or None), C.c_void_p(param or None),
                                C.byref(out) if out is not None else None, None)


def test_invalid_arguments_are_refused_without_a_device():
    assert _call(None) == 1
    assert _call(_spec(), draws=0) == 1
    assert _call(_spec(), outputs=None) == 1
    assert _call(_spec(), outputs=(0, 0, COUNTS)) == 1                          # neither scores nor ranks
    assert _call(_spec(kind=1), param=0) == 1
    assert _call(_spec(kind=2), param=0, outputs=(OUT, 0, COUNTS)) == 1
    assert _call(_spec(kind=2)) == 1                                             # the indicator has no ranks
    assert _call(_spec(kind=3)) == 1
    assert _call(_spec(kind=2**63)) == 1
    assert _call(_spec(split=2)) == 1
    assert _call(_spec(dim=0)) == 1
    assert _call(_spec(n_chains=0)) == 1
    assert _call(_spec(n_draws=0)) == 1
    assert _call(_spec(n_draws=1, split=1)) == 1                                 # n = 0: the only draw is the middle one
    assert _call(_spec(n_draws=2**16, n_chains=2**15)) == 1                      # n = 2^31
    assert _call(_spec(n_draws=2**31 + 1, n_chains=1)) == 1                      # odd, split: n = 2^31
    assert _call(_spec(n_draws=2**30, n_chains=4, ids=[1, 3])) == 1
    assert _call(_spec(n_draws=1, n_chains=1, dim=2**31, split=0)) == 1
    assert _call(_spec(ids=[])) == 1                                             # empty
    assert _call(_spec(ids=[0, 2, 2])) == 1                                      # not strictly increasing
    assert _call(_spec(ids=[2, 1])) == 1
    assert _call(_spec(ids=[0, 4])) == 1                                         # out of range
    nbytes = 20 * 4 * 3 * 8
    assert _call(_spec(), outputs=(DRAWS, RANKS, COUNTS)) == 1                   # in place
    assert _call(_spec(), outputs=(DRAWS + nbytes - 8, RANKS, COUNTS)) == 1      # the last word of the trace
    assert _call(_spec(), outputs=(DRAWS - nbytes + 8, RANKS, COUNTS)) == 1      # the output's last word is the trace's first
    assert _call(_spec(ids=[1, 3]), outputs=(DRAWS - nbytes // 2 + 8, 0, 0)) == 1          # (the output is compact: half as long)
    assert b"nm_transform_draws" in N.load_library().nm_transform_last_error()
    L, z = N.load_library(), C.c_double(7.0)
    for n, r2 in ((0, 2), (2**31, 2), (5, 1), (5, 0), (5, 11), (2**31 - 1, 2**32 - 1)):
        assert L.nm_rank_normal_score(n, r2, C.byref(z)) == 1 and z.value == 7.0, (n, r2)
    assert L.nm_rank_normal_score(5, 6, None) == 1
    assert L.nm_rank_normal_score(2**31 - 1, 2**32 - 2, C.byref(z)) == 0 and z.value > 6.0


def _twin(n, r2):
    z = C.c_double()
    assert N.load_library().nm_rank_normal_score(n, r2, C.byref(z)) == 0
    return z.value


def test_score_twin_against_mpmath():
    """Phi^-1 at u = (4 rank2 - 3) / (8 n + 2), exact in mpmath at 40 digits.  Bound 2e-15 relative: 3.5 x the 5.7e-16 a numpy
    transcription of the same algorithm with libm's log shows on this grid (AS241's own error plus the roundings of the evaluation);
    the margin is for dlog rounding its last bit differently from libm.  Nothing downstream needs better than 1e-12."""
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.RandomState(241)
    worst, worst_np = 0.0, 0.0
    for n in (1, 2, 3, 10, 1000, 2**20, 2**31 - 1):
        r2s = {r for r in (2, 3, 4, n, n + 1, 2 * n - 1, 2 * n) if 2 <= r <= 2 * n}
        r2s |= set(rng.randint(2, 2 * n + 1, size=300, dtype=np.int64).tolist())
        for r2 in sorted(r2s):
            u = mpmath.mpf(4 * r2 - 3) / mpmath.mpf(8 * n + 2)
            want = mpmath.sqrt(2) * mpmath.erfinv(2 * u - 1)
            got = _twin(n, r2)
            if r2 == n + 1:
                assert got == 0.0 and want == 0
                continue
            err = float(abs((mpmath.mpf(got) - want) / want))
            worst = max(worst, err)
            worst_np = max(worst_np, float(abs((mpmath.mpf(float(rank_ref.score_numpy(n, r2))) - want) / want)))
            assert err <= 2e-15, (n, r2, got, float(want), err)
    print(f"score twin: worst relative error {worst:.3e} (the numpy transcription with libm's log: {worst_np:.3e})")


def test_score_is_antisymmetric_centred_and_monotone():
    for n in (1, 2, 3, 10, 1000, 2**20, 2**31 - 1):
        assert np.float64(_twin(n, n + 1)).view(np.uint64) == 0                            # +0.0 exactly
        rng = np.random.RandomState(n % 1000)
        for r2 in [2, 3, n, 2 * n] + rng.randint(2, 2 * n + 1, size=200, dtype=np.int64).tolist():
            if not 2 <= r2 <= 2 * n or r2 == n + 1:
                continue
            a, b = np.float64(_twin(n, r2)), np.float64(-_twin(n, 2 * n + 2 - r2))
            assert a.view(np.uint64) == b.view(np.uint64), (n, r2)
    z = np.array([_twin(1000, r2) for r2 in range(2, 2001)])
    assert (np.diff(z) >= 0).all() and z[0] < -3.0 and z[-1] > 3.0


def _rank2(values, kind=0, centre=None):
    x = np.asarray(values, dtype=np.float64).reshape(-1, 1, 1)
    out, r2, nan = rank_ref.transform(x, kind, None if centre is None else [centre], split=False)
    return out[:, 0, 0], r2[:, 0, 0].tolist(), int(nan[0])


def test_restated_ranks_against_scipy():
    """equal to scipy.stats.rankdata(method="average") wherever no -0.0 meets a +0.0"""
    from scipy.stats import rankdata
    rng = np.random.default_rng(11)
    for shape in ((40, 7, 3), (1, 1, 2), (33, 5, 4)):
        x = rng.normal(size=shape)                                                         # tie-free
        _, r2, nan = rank_ref.transform(x, 0, split=False)
        want = np.stack([rankdata(x[:, :, d].reshape(-1), method="average").reshape(shape[:2]) for d in range(shape[2])], axis=2)
        assert (r2 == 2 * want).all() and (nan == 0).all() and r2.dtype == np.uint32
        t = rng.integers(-2, 3, size=shape).astype(np.float64) + 0.0                       # heavy ties (no negative zero: -0.0 + 0.0 = +0.0)
        _, r2, _ = rank_ref.transform(t, 0, split=False)
        want = np.stack([rankdata(t[:, :, d].reshape(-1), method="average").reshape(shape[:2]) for d in range(shape[2])], axis=2)
        assert (r2 == 2 * want).all()
    ids = [0, 2, 5]
    x = rng.normal(size=(12, 7, 2))
    _, r2, _ = rank_ref.transform(x, 0, split=False, chain_ids=ids)
    assert r2.shape == (12, 3, 2) and (r2[:, :, 1] == 2 * rankdata(x[:, ids, 1].reshape(-1)).reshape(12, 3)).all()
    # the folded kind ranks |x - c|
    c = np.array([0.25, -1.0])
    _, r2, _ = rank_ref.transform(x, 1, c, split=False)
    assert (r2[:, :, 0] == 2 * rankdata(np.abs(x[:, :, 0] - 0.25).reshape(-1)).reshape(12, 7)).all()


def test_special_columns_by_hand():
    # both zeros are distinct keys, -0.0 below +0.0 (scipy would tie all five at rank 3): the two -0.0 share ranks 1, 2, the +0.0 ranks 3, 4, 5
    _, r2, _ = _rank2([0.0, -0.0, 0.0, -0.0, 0.0])
    assert r2 == [8, 3, 8, 3, 8]
    # +-inf are ordinary ends of the order
    z, r2, nan = _rank2([2.0, np.inf, -np.inf, 1.0, np.inf])
    assert r2 == [6, 9, 2, 4, 9] and nan == 0 and z[2] == _twin(5, 2) and z[1] == z[4] == _twin(5, 9)
    # subnormals of both signs
    t = 5e-324
    _, r2, _ = _rank2([t, -t, 2 * t, -3 * t, 0.0])
    assert r2 == [8, 4, 10, 2, 6]
    # all equal: every rank2 = n + 1, every score +0.0
    z, r2, _ = _rank2([2.5] * 7)
    assert r2 == [8] * 7 and (z.view(np.uint64) == 0).all()
    # a NaN (either sign): the whole column NaN, rank2 0, the count exact
    z, r2, nan = _rank2([1.0, np.nan, 3.0, -np.nan])
    assert np.isnan(z).all() and r2 == [0] * 4 and nan == 2
    # the fold: |x - 2| of (0, 1, 2, 3, 4) is (2, 1, 0, 1, 2): exact ties of symmetric pairs, the centre itself the smallest
    z, r2, _ = _rank2([0.0, 1.0, 2.0, 3.0, 4.0], kind=1, centre=2.0)
    assert r2 == [9, 5, 2, 5, 9] and z[0] == z[4] == _twin(5, 9) and z[2] == _twin(5, 2)
    z, r2, nan = _rank2([0.0, np.inf, 1.0], kind=1, centre=np.inf)                          # inf - inf: a NaN the fold makes
    assert nan == 1 and r2 == [0, 0, 0]
    # odd N with split: the middle draw is NaN / 0 and is not counted in n
    x = np.arange(10.0).reshape(5, 2, 1)
    out, r2, nan = rank_ref.transform(x, 0, split=True)
    assert np.isnan(out[2]).all() and (r2[2] == 0).all() and nan[0] == 0
    assert r2[[0, 1, 3, 4], :, 0].reshape(-1).tolist() == [2, 4, 6, 8, 10, 12, 14, 16]      # n = 8
    assert out[0, 0, 0] == _twin(8, 2) and out[4, 1, 0] == _twin(8, 16)
    out, r2, _ = rank_ref.transform(x, 0, split=False)
    assert r2[:, :, 0].reshape(-1).tolist() == list(range(2, 22, 2)) and out[2, 0, 0] == _twin(10, 10)
    # the indicator: IEEE <=, a NaN element is NaN and counted, a NaN threshold takes the column, every row is written
    x = np.array([1.0, 2.0, -0.0, np.nan, 3.0, 0.0]).reshape(3, 2, 1).repeat(3, axis=2)
    out, r2, nan = rank_ref.transform(x, 2, [2.0, 0.0, np.nan], split=True)
    assert r2 is None and nan.tolist() == [1, 1, 1]
    assert np.array_equal(out[:, :, 0].reshape(-1), [1, 1, 1, np.nan, 0, 1], equal_nan=True)
    assert np.array_equal(out[:, :, 1].reshape(-1), [0, 0, 1, np.nan, 0, 1], equal_nan=True)       # -0.0 <= +0.0
    assert np.isnan(out[:, :, 2]).all()


def _point_draws():
    """1000 draws x 4 chains: column 0 the fourth chain with 3 x the sd of the others (same location), column 1 iid Cauchy"""
    rng = np.random.RandomState(20261020)
    x = np.empty((1000, 4, 2))
    x[:, :, 0] = rng.standard_normal((1000, 4)) * np.array([1.0, 1.0, 1.0, 3.0])
    x[:, :, 1] = rng.standard_cauchy((1000, 4))
    return x


def test_rank_normalisation_sees_what_the_classic_rhat_cannot():
    x = _point_draws()
    classic = summary_ref.summarize(x, True, 32)
    rd = rank_ref.rank_diagnostics(x, True, 32)
    n = 4000.0
    print("classic rhat", classic.rhat, "rhat_rank", rd.rhat_rank, "ess_bulk / n", rd.ess_bulk / n, "ess_tail / n", rd.ess_tail / n)
    assert classic.rhat[0] < 1.01 and rd.rhat_rank[0] > 1.05                               # scale differs, location agrees
    assert 0.8 <= rd.ess_bulk[1] / n <= 1.35                                               # heavy tails: iid is iid
    assert (rd.nan_count == 0).all()


def test_bulk_ess_on_the_ar1_input():
    x, rhos = summary_ref.ar1_draws()
    rd = rank_ref.rank_diagnostics(x, True, 32)
    ratio = rd.ess_bulk / (x.shape[0] * x.shape[1] * (1 - rhos) / (1 + rhos))
    print("bulk ess ratios", ratio, "truncated", rd.ess_bulk_truncated)
    assert rd.ess_bulk_truncated[3] == 1                                                   # rho = 0.9 runs out of lags
    for j in np.flatnonzero(rd.ess_bulk_truncated == 0):
        assert 0.8 <= ratio[j] <= 1.35, (j, ratio[j])
    assert (rd.ess_bulk_truncated[[0, 1, 2, 4]] == 0).all()
