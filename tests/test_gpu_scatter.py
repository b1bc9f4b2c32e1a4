"""nm_pooled_scatter on the device against the restatement of its definition (tests/scatter_ref.py): BIT equality (a NaN compares as a
NaN), over the shapes at which the kernel takes another path — dims around the 16-wide MFMA block and the 64-wide macro tile, 8- and
16-byte lane loads, one slab, ragged slabs, a last slab of one row, row counts past the slab clamp — and over what the rows hold."""
import ctypes as C

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import scatter_ref
from test_scatter_cpu import generic

pytestmark = pytest.mark.gpu


def bits(a):
    """NaN compared as NaN: every NaN is one value, everything else its own bits"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def device_scatter(x, center, stats=None, misalign=False, want_count=True):
    """the raw call on buffers this test lays out itself; misalign: the rows start 8 bytes past a 16-byte boundary"""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, dim = x.shape
    buf = torch.empty(x.size + 2, dtype=torch.float64, device="cuda")
    off = (0 if buf.data_ptr() % 16 == 0 else 1) + (1 if misalign else 0)
    rows = buf[off:off + x.size]
    rows.copy_(torch.from_numpy(x.reshape(-1)))
    assert rows.data_ptr() % 16 == (8 if misalign else 0)
    c = torch.from_numpy(np.ascontiguousarray(center, dtype=np.float64)).cuda()
    st = None if stats is None else torch.from_numpy(np.ascontiguousarray(stats).view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full((dim, dim), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L = N.load_library()
    _lib.check_status(L.nm_pooled_scatter(n, dim, rows.data_ptr(), c.data_ptr(), None if st is None else st.data_ptr(), out.data_ptr(),
                                          cnt.data_ptr() if want_count else None, None), L.nm_pooled_last_error)
    torch.cuda.synchronize()
    return out.cpu().numpy(), float(cnt.item())


def check(x, center, stats=None, **kw):
    want, want_count = scatter_ref.scatter(x, center, stats)
    got, count = device_scatter(x, center, stats, **kw)
    assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:5]
    assert (bits(got) == bits(got.T)).all()
    if kw.get("want_count", True):
        assert count == want_count
    return got


# (n_rows, dim): the smallest shapes; dims 15 / 16 / 17 around the MFMA block; 65 = one more than the macro tile's width, 130 = three
# macro tiles a side (six blocks per slab, off-diagonal ones included); an odd dim; 300 rows = two slabs, the second ragged
SHAPES = [(1, 1), (4, 1), (5, 16), (300, 15), (300, 16), (300, 17), (300, 65), (90, 130), (37, 33), (260, 2)]


@pytest.mark.parametrize("n,dim", SHAPES)
def test_shapes_bit_exact(n, dim):
    rng = np.random.default_rng(1000 * n + dim)
    x = generic(rng, n, dim)
    check(x, np.zeros(dim))
    check(x, x.mean(axis=0))


@pytest.mark.parametrize("n,dim", [(37, 33), (300, 17), (300, 16), (5, 2)])
def test_rows_on_a_pointer_aligned_to_8_bytes_only(n, dim):
    """8-byte lane loads: an odd dim, and an even dim whose rows start 8 bytes past a 16-byte boundary — the same bits as the 16-byte loads"""
    rng = np.random.default_rng(n + dim)
    x = generic(rng, n, dim)
    a = check(x, x.mean(axis=0), misalign=True)
    b = check(x, x.mean(axis=0), misalign=False)
    assert (bits(a) == bits(b)).all()


# one slab; four slabs, the last ragged (R = 252, 244 rows); a last slab of ONE row at the clamp (n = 63 R + 1, R = 256); past the clamp
# (n > 256 * 64: the slabs grow instead of multiplying); a last slab whose rows end inside a 32-row panel and inside an MFMA's four rows
SLABS = [(200, 8), (1000, 8), (256 * 63 + 1, 8), (256 * 64 + 117, 8), (522, 8)]


@pytest.mark.parametrize("n,dim", SLABS)
def test_slab_edges_bit_exact(n, dim):
    k, R = scatter_ref.slabs(n)
    assert {200: (1, 200), 1000: (4, 252), 16129: (64, 256), 16501: (64, 260), 522: (3, 176)}[n] == (k, R)
    rng = np.random.default_rng(n)
    x = generic(rng, n, dim)
    check(x, x.mean(axis=0))


def test_rows_left_out_are_selected_away():
    """a statistics buffer that leaves rows out; the rows left out hold NaN (a failed chain's do) and the result is finite"""
    rng = np.random.default_rng(21)
    for n, dim in ((300, 17), (1000, 8), (90, 66)):
        x = generic(rng, n, dim)
        st = scatter_ref.stats_rows(n, rng)
        keep = scatter_ref.kept(st, n)
        assert 0 < keep.sum() < n
        x[~keep] = np.nan
        got = check(x, np.nanmean(x, axis=0), st)
        assert np.isfinite(got).all()
    # every row left out: S = 0, count 0
    st = np.zeros(40, dtype=N.STATS_DTYPE)
    got = check(np.full((40, 5), np.nan), np.zeros(5), st)
    assert (bits(got) == 0).all()


def test_a_nan_in_a_kept_row_stays_in_its_row_and_column():
    rng = np.random.default_rng(22)
    n, dim = 300, 70
    x = generic(rng, n, dim)
    x[123, 66] = np.nan
    x[7, 3] = np.inf
    got = check(x, np.zeros(dim))
    nan = np.isnan(got)
    expect = np.zeros((dim, dim), dtype=bool)
    expect[66, :] = expect[:, 66] = True
    assert (nan == expect).all()
    assert np.isinf(got[3, 3]) and np.isinf(np.delete(got[3], 66)).all()


def test_count_may_be_null_and_a_repeat_gives_the_same_bits():
    rng = np.random.default_rng(23)
    x = generic(rng, 700, 40)
    c = x.mean(axis=0)
    a = check(x, c)
    b = check(x, c, want_count=False)
    d, _ = device_scatter(x, c)
    assert (bits(a) == bits(b)).all() and (bits(a) == bits(d)).all()


def test_front_end_tensor_against_array():
    import torch
    rng = np.random.default_rng(24)
    x = generic(rng, 12 * 25, 10).reshape(12, 25, 10)
    st = scatter_ref.stats_rows(300, rng).reshape(12, 25)
    c = x.reshape(-1, 10).mean(axis=0)
    want, want_count = scatter_ref.scatter(x, c, st)
    S_a, n_a = N.pooled_scatter(x, c, stats=st)
    assert isinstance(S_a, np.ndarray) and n_a == want_count and (bits(S_a) == bits(want)).all()
    xt, ct = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    stt = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    S_t, n_t = N.pooled_scatter(xt, ct, stats=stt, stream=side)
    side.synchronize()
    assert isinstance(S_t, torch.Tensor) and S_t.is_cuda and float(n_t.item()) == want_count
    assert (bits(S_t.cpu().numpy()) == bits(want)).all()
    S_all, n_all = N.pooled_scatter(xt, ct)
    torch.cuda.synchronize()
    assert float(n_all.item()) == 300 and (bits(S_all.cpu().numpy()) == bits(scatter_ref.scatter(x, c)[0])).all()
    with pytest.raises(ValueError):
        N.pooled_scatter(x, c[:-1])
    with pytest.raises(N.NutsAmdError):
        N.pooled_scatter(np.zeros((3, N.NM_SCATTER_MAX_DIM + 1)), np.zeros(N.NM_SCATTER_MAX_DIM + 1))


@pytest.mark.parametrize("shape", [(50, 8, 6), (20, 33, 17), (3, 2, 70)])
def test_covariance_draws_against_numpy(shape):
    """|cov - np.cov| <= (2 n + 12) 2^-53 sum_r |y_ri y_rj| / (n - 1) per entry.  Derived: this side's scatter is within (n + 4) units of
    2^-53 sum |y y| of the exact one (scatter_ref.scatter_bound), numpy's centred product within n + 4 of them as well (a rounding per y, at
    most one per term of a dot product of n terms whatever its order), each division by n - 1 adds one, and the two sides' means differ
    from the exact one by roundings whose effect on a scatter ABOUT the mean is of second order (n delta delta')."""
    rng = np.random.default_rng(sum(shape))
    x = generic(rng, shape[0] * shape[1], shape[2]).reshape(shape)
    mean, cov, count = N.covariance_draws(x)
    flat = x.reshape(-1, shape[2])
    n = flat.shape[0]
    assert count == n and cov.shape == (shape[2], shape[2]) and (cov == cov.T).all()
    assert np.abs(mean - flat.mean(axis=0)).max() <= n * 2.0**-53 * np.abs(flat).max()
    y = np.abs(flat - flat.mean(axis=0))
    bound = (2 * n + 12) * 2.0**-53 * (y.T @ y) / (n - 1)
    assert (np.abs(cov - np.cov(flat, rowvar=False)) <= bound).all()
    import torch
    mean_t, cov_t, count_t = N.covariance_draws(torch.from_numpy(x).cuda())
    assert count_t == n and (bits(cov_t) == bits(cov)).all() and (bits(mean_t) == bits(mean)).all()
    # only the rows the pooled adaptation keeps
    st = scatter_ref.stats_rows(n, rng)
    keep = scatter_ref.kept(st, n)
    if keep.sum() > 2:
        mean_k, cov_k, count_k = N.covariance_draws(x, stats=st)
        yk = np.abs(flat[keep] - flat[keep].mean(axis=0))
        assert count_k == keep.sum()
        assert (np.abs(cov_k - np.cov(flat[keep], rowvar=False)) <= (2 * count_k + 12) * 2.0**-53 * (yk.T @ yk) / (count_k - 1)).all()


def test_front_end_queues_its_own_copies_on_the_callers_stream():
    """a non-contiguous tensor and a host centre on a side stream: the copies the call makes are ordered before its kernel"""
    import torch
    rng = np.random.default_rng(25)
    n, dim = 20000, 16
    wide = generic(rng, n, 2 * dim)
    x = np.ascontiguousarray(wide[:, ::2])
    c = x.mean(axis=0)
    want, _ = scatter_ref.scatter(x, c)
    view = torch.from_numpy(wide).cuda()[:, ::2]
    assert not view.is_contiguous()
    side = torch.cuda.Stream()
    S, cnt = N.pooled_scatter(view, c, stream=side)
    side.synchronize()
    assert float(cnt.item()) == n and (bits(S.cpu().numpy()) == bits(want)).all()
