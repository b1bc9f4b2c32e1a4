"""nm_summarize_draws on the GPU (csrc/summary.hip): every output equals the numpy restatement of the definition (tests/summary_ref.py)
BIT FOR BIT — NaNs compared as NaNs, their payloads not — on the smallest shapes that cross each boundary of the kernels: the minimum
size, an odd number of draws, a ragged chunk of 32 series, a ragged column tile, every lag bucket, 8- and 16-byte lanes, selected
chains, absent outputs, a constant column and a column with an Inf.  Then the Python front end and ChainBatch.draw_summary end to end."""
import ctypes as C

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import summary_ref

pytestmark = pytest.mark.gpu


def generic(shape, seed):
    """generic doubles: normal, scaled by exp(U(-3, 3)) per column, plus a per-column offset"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape) * np.exp(rng.uniform(-3, 3, size=shape[2])) + rng.normal(size=shape[2]) * 10.0


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def assert_equals_ref(got, want, fields=summary_ref.FIELDS):
    assert got.n_series == want.n_series and got.n_per_series == want.n_per_series
    for f in fields:
        g, w = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        if not same_bits(g, w):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w)))) if g.shape == w.shape else None
            raise AssertionError(f"{f}: device and restatement differ, first at {None if bad is None else bad[:3].tolist()}: "
                                 f"{g.ravel()[:4]} vs {w.ravel()[:4]}")


CASES = [
    # (N, C, D), split, max_lag
    ((4, 1, 1), True, 32),            # the minimum: M = 2, n = 2, L = 1
    ((7, 3, 1), True, 32),            # odd N: the middle draw belongs to neither half
    ((40, 33, 130), False, 32),       # ragged chunk of 32, dim ragged over a 128-wide block; 32 lags: 8-byte lanes, three column tiles
    ((40, 33, 130), True, 32),        # L = 19
    ((40, 33, 130), True, 16),        # 16-byte lanes on a wide row: two tiles of 33 lanes, the 16-lag kernel
    ((40, 33, 130), False, 8),        # ... the 8-lag kernel
    ((64, 70, 5), True, 64),          # L clamps to n - 1 = 31; odd dim: 8-byte lanes, 12 series side by side
    ((30, 40, 10), True, 1),
    ((30, 40, 10), True, 7),          # odd L
    ((140, 3, 6), False, 64),         # the 64-lag kernel
    ((24, 35, 101), True, 9),         # two column tiles of an odd dim, the 16-lag kernel
]


@pytest.mark.parametrize("shape,split,max_lag", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{'split' if sp else 'whole'}-lag{l}" for s, sp, l in CASES])
def test_device_equals_restatement(shape, split, max_lag):
    x = generic(shape, seed=sum(shape) + max_lag)
    got = N.summarize_draws(x, split=split, max_lag=max_lag)
    assert_equals_ref(got, summary_ref.summarize(x, split=split, max_lag=max_lag))
    assert got.autocorr.shape[0] == min(max_lag, got.n_per_series - 1) + 1


@pytest.fixture(scope="module")
def thirds():
    x = generic((50, 100, 3), seed=5)
    ids = np.arange(0, 100, 3)
    return x, ids, summary_ref.summarize(x, split=True, max_lag=32, chain_ids=ids)


def test_selected_chains_all_outputs(thirds):
    x, ids, want = thirds
    assert_equals_ref(N.summarize_draws(x, chain_ids=ids), want)
    assert want.n_series == 2 * len(ids)


def test_selected_chains_only_ess_requested(thirds):
    import torch
    x, ids, want = thirds
    t = torch.from_numpy(x).cuda()
    ess = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    keep = np.ascontiguousarray(ids, dtype=np.uint64)
    spec = _lib.NmSummarySpec(50, 100, 3, 1, 32, len(keep), keep.ctypes.data)
    out = _lib.NmSummaryOutputs()
    out.d_ess = ess.data_ptr()
    torch.cuda.synchronize()
    L = N.load_library()
    _lib.check_status(L.nm_summarize_draws(C.byref(spec), C.c_void_p(t.data_ptr()), C.byref(out), None), L.nm_summary_last_error)
    torch.cuda.synchronize()
    assert same_bits(ess.cpu().numpy(), want.ess)


def test_trace_aligned_to_8_bytes_only():
    """an even dim whose trace starts 8 bytes off a 16-byte boundary (the raw ABI; torch's own allocations never do): 8-byte lanes"""
    import torch
    shape = (30, 7, 12)
    x = generic(shape, seed=21)
    buf = torch.empty(x.size + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:] = torch.from_numpy(x.ravel()).cuda()
    D, n, M = 12, 15, 14
    outs = {k: torch.empty(s, dtype=torch.int64 if k == "ess_truncated" else torch.float64, device="cuda")
            for k, s in dict(mean=(D,), sd=(D,), within_var=(D,), rhat=(D,), ess=(D,), ess_truncated=(D,), autocorr=(8, D),
                             chain_mean=(M, D), chain_var=(M, D)).items()}
    out = _lib.NmSummaryOutputs()
    for k, b in outs.items():
        setattr(out, "d_" + k, b.data_ptr())
    spec = _lib.NmSummarySpec(30, 7, 12, 1, 7, 0, None)
    torch.cuda.synchronize()
    L = N.load_library()
    _lib.check_status(L.nm_summarize_draws(C.byref(spec), C.c_void_p(buf.data_ptr() + 8), C.byref(out), None), L.nm_summary_last_error)
    torch.cuda.synchronize()
    want = summary_ref.summarize(x, max_lag=7)
    for f in summary_ref.FIELDS:
        got = outs[f].cpu().numpy()
        assert same_bits(got.astype(np.uint64) if f == "ess_truncated" else got, getattr(want, f)), f


def test_constant_column_and_inf_column():
    x = generic((20, 5, 4), seed=9)
    x[:, :, 1] = 2.5                    # constant: W = 0, var_plus = 0 -> NaN rhat and ess
    x[13, 2, 3] = np.inf
    got, want = N.summarize_draws(x, max_lag=6), summary_ref.summarize(x, max_lag=6)
    assert_equals_ref(got, want)
    assert np.isnan(got.rhat[1]) and np.isnan(got.ess[1]) and np.isnan(want.rhat[1]) and np.isnan(want.ess[1])
    assert np.isfinite(got.rhat[[0, 2]]).all() and not np.isfinite(got.mean[3])


def test_ar1_bits_flags_and_bands():
    x, _ = summary_ref.ar1_draws()
    assert_equals_ref(N.summarize_draws(x), summary_ref.summarize(x))
    summary_ref.check_ar1_bands(lambda a, split, lag: N.summarize_draws(a, split=split, max_lag=lag))


def test_tensor_and_array_inputs_agree():
    import torch
    x = generic((30, 9, 8), seed=2)
    a = N.summarize_draws(x, max_lag=5)
    t = torch.from_numpy(x).cuda()
    b = N.summarize_draws(t, max_lag=5)
    c = N.summarize_draws(torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda().permute(1, 0, 2), max_lag=5)   # not contiguous
    for f in summary_ref.FIELDS:
        assert same_bits(getattr(a, f), getattr(b, f)) and same_bits(getattr(a, f), getattr(c, f)), f
    assert (t.cpu().numpy() == x).all()                            # summarised where it lies, unchanged


def _warm_batch(logp, chains, tune, seed):
    b = N.ChainBatch(N.DiagNutsSettings(num_chains=chains, seed=seed, num_tune=tune), logp, chains)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    b.draw_device(tune)
    return b


def test_draw_summary_end_to_end_positions():
    logp = N.LogpSpec.diag_normal(np.exp(np.linspace(-2.0, 2.0, 40)))
    b = _warm_batch(logp, 256, 300, seed=17)
    got, st = b.draw_summary(100)
    b.close()
    b = _warm_batch(logp, 256, 300, seed=17)
    pos, st2 = b.draw_many(100)
    b.close()
    assert st.shape == (100, 256) and st.tobytes() == st2.tobytes()
    assert_equals_ref(got, summary_ref.summarize(pos))
    assert got.n_series == 512 and got.n_per_series == 50
    assert (np.abs(got.mean) < 0.1 * got.sd).all() and (got.rhat < 1.05).all()


def test_draw_summary_end_to_end_expanded():
    logp = N.LogpSpec.eight_schools()
    b = _warm_batch(logp, 256, 300, seed=18)
    got, st = b.draw_summary(100, expanded=True, max_lag=16)
    b.close()
    b = _warm_batch(logp, 256, 300, seed=18)
    ex = b.expanded_draw_many(100, vectors=(), expanded=True)[3]
    b.close()
    assert_equals_ref(got, summary_ref.summarize(ex, max_lag=16))
    assert (st["chain_status"] == 0).all()


def test_chain_that_failed_at_set_position_is_left_out():
    def normal(chain, x):
        return -0.5 * float(np.dot(x, x)), -x
    s = N.DiagNutsSettings(num_chains=5, seed=3, num_tune=10)
    runs = []
    for _ in range(2):
        b = N.ChainBatch(s, N.LogpSpec.host_callback(3, normal, threads=2), 5)
        x0 = b.init_positions_uniform()
        x0[2] = np.nan
        assert list(b.set_position(x0, raise_on_error=False)) == [0, 0, 1, 0, 0]
        runs.append(b)
    got, st = runs[0].draw_summary(24, max_lag=4)
    pos, _ = runs[1].draw_many(24, raise_on_error=False)
    for b in runs:
        b.close()
    assert got.n_series == 2 * 4 and got.chain_mean.shape == (8, 3)
    assert_equals_ref(got, summary_ref.summarize(pos, max_lag=4, chain_ids=[0, 1, 3, 4]))
    assert (st["n_steps"][:, 2] == 0).all() and (st["n_steps"][:, [0, 1, 3, 4]] > 0).all()
