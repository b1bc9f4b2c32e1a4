"""nm_quantile_draws on the GPU (csrc/quantile.hip): the quantiles and the NaN counts equal the numpy restatement of the definition
(tests/quantile_ref.py) BIT FOR BIT — NaNs compared as NaNs — on the smallest shapes that cross each boundary of the kernels: the
minimum size, 8- and 16-byte lanes, several rows side by side, a ragged column tile, more rows than one block's slab, a misaligned base;
on columns made to defeat single passes of the selection; for every kind of probability list.  Then the front ends."""
import ctypes as C

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import quantile_ref

pytestmark = pytest.mark.gpu

P3 = [0.05, 0.5, 0.95]
P16 = [0.0, 0.01, 0.025, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.5, 2.0 / 3.0, 0.75, 0.9, 0.95, 0.975, 0.99, 1.0]
PROBS = {"median": [0.5], "ends": [0.0, 1.0], "unsorted-repeat": [0.9, 0.1, 0.5, 0.1], "sixteen": P16}


def generic(shape, seed):
    """generic doubles: normal, scaled by exp(U(-3, 3)) per column, plus a per-column offset"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape) * np.exp(rng.uniform(-3, 3, size=shape[2])) + rng.normal(size=shape[2]) * 10.0


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def assert_equals_ref(x, probs, chain_ids=None, got=None):
    q, nan = got if got is not None else N.quantile_draws(x, probs, chain_ids=chain_ids)
    wq, wnan = quantile_ref.quantile(x, probs, chain_ids=chain_ids)
    assert same_bits(nan, wnan), f"nan_count: {nan} vs {wnan}"
    if not same_bits(q, wq):
        bad = np.argwhere(~((q == wq) | (np.isnan(q) & np.isnan(wq)))) if q.shape == wq.shape else None
        raise AssertionError(f"device and restatement differ, first at [prob, column] {None if bad is None else bad[:4].tolist()}: "
                             f"{None if bad is None else [(q[i, j], wq[i, j]) for i, j in bad[:4]]}")
    return q, nan


SHAPES = [
    (1, 1, 1),             # n = 1
    (2, 1, 1),
    (5, 3, 7),             # odd dim: 8-byte lanes
    (17, 70, 10),          # K4's row: several rows per wavefront, 16-byte lanes
    (40, 33, 130),         # ragged over the column tiles
    (300, 5, 3),           # more rows than one block's slab
]


@pytest.mark.parametrize("pname", list(PROBS))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_device_equals_restatement(shape, pname):
    assert_equals_ref(generic(shape, seed=sum(shape)), PROBS[pname])


def hard_columns(n_draws, n_chains, seed):
    """one column per way a pass of the selection can fail to narrow anything, between two generic columns"""
    rng = np.random.default_rng(seed)
    n = n_draws * n_chains
    x = generic((n_draws, n_chains, 12), seed).reshape(n, 12)
    x[:, 1] = -3.75                                                                   # all equal: no pass narrows anything
    x[:, 2] = np.where(rng.random(n) < 0.3, 1.0, -2.0)                                # two distinct values
    base = np.float64(1.2345678).view(np.uint64) & ~np.uint64(0xFF)
    x[:, 3] = (base | rng.integers(0, 256, size=n).astype(np.uint64)).view(np.float64)          # the top 56 bits agree: the last pass decides
    mant = np.uint64(0x000F_1234_5678_9ABC)                                           # only the sign and the top byte differ
    top = (rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(56))
    x[:, 4] = (top | mant).view(np.float64)                                           # (bits 52 - 55 are zero: no exponent of all ones)
    x[:, 5] = rng.choice([-1e-3, -0.0, 0.0, 1e-3, -5e-324, 5e-324], size=n)           # mixed signs around zero, both zeros
    x[:, 6] = rng.choice([-np.inf, np.inf, -1.0, 0.5, 2.0], size=n, p=[0.2, 0.2, 0.2, 0.2, 0.2])
    x[:, 7] = rng.integers(-40, 40, size=n) * 5e-324                                  # subnormals of both signs
    x[:, 8] = rng.integers(0, 3, size=n).astype(np.float64)                           # heavy ties
    x[:, 9] = np.arange(n, dtype=np.float64)[rng.permutation(n)]                      # a permutation: every rank is its own value
    return np.ascontiguousarray(x.reshape(n_draws, n_chains, 12))


@pytest.mark.parametrize("pname", list(PROBS))
def test_columns_that_defeat_single_passes(pname):
    x = hard_columns(40, 13, seed=4)
    assert np.isfinite(x[:, :, 4]).all() and len(np.unique(x[:, :, 3])) > 100
    assert_equals_ref(x, PROBS[pname])


def test_probabilities_with_integer_positions():
    x = hard_columns(21, 5, seed=6)                  # n - 1 = 104 = 8 * 13
    probs = [0.125, 0.25, 0.5, 0.875, 1.0 / 13.0]
    assert all(quantile_ref.ranks(p, 105)[2] == 0.0 for p in probs[:4])
    assert_equals_ref(x, probs)


def test_nan_column_next_to_clean_ones():
    x = generic((30, 7, 6), seed=8)
    clean, _ = N.quantile_draws(x, P3)
    x[3, 2, 1] = np.nan
    x[29, 6, 1] = -np.nan
    x[:, :, 4] = np.nan
    q, nan = assert_equals_ref(x, P3)
    assert nan.tolist() == [0, 2, 0, 0, 210, 0] and nan.dtype == np.uint64
    assert np.isnan(q[:, [1, 4]]).all() and same_bits(q[:, [0, 2, 3, 5]], clean[:, [0, 2, 3, 5]])


@pytest.fixture(scope="module")
def thirds():
    x = generic((50, 100, 3), seed=5)
    x[7, 4, 2] = np.nan                              # a chain that is left out: its NaN must not count
    x[9, 3, 1] = np.nan                              # a chain that is selected
    return x, np.arange(0, 100, 3)


def test_selected_chains(thirds):
    x, ids = thirds
    q, nan = assert_equals_ref(x, P3, chain_ids=ids)
    assert nan.tolist() == [0, 1, 0] and np.isfinite(q[:, [0, 2]]).all()


def _raw_call(ptr, shape, probs, want_q=True, want_nan=True):
    """the C ABI on a device pointer: (quantiles or None, nan_count or None)"""
    import torch
    n_draws, n_chains, dim = shape
    p = np.ascontiguousarray(probs, dtype=np.float64)
    q = torch.full((len(p), dim), -7.0, dtype=torch.float64, device="cuda")
    nan = torch.full((dim,), -7, dtype=torch.int64, device="cuda")
    spec = _lib.NmQuantileSpec(n_draws, n_chains, dim, len(p), p.ctypes.data, 0, None)
    out = _lib.NmQuantileOutputs(q.data_ptr() if want_q else None, nan.data_ptr() if want_nan else None)
    torch.cuda.synchronize()
    L = N.load_library()
    _lib.check_status(L.nm_quantile_draws(C.byref(spec), C.c_void_p(ptr), C.byref(out), None), L.nm_quantile_last_error)
    torch.cuda.synchronize()
    return q.cpu().numpy(), nan.cpu().numpy()


def test_each_output_absent_in_turn():
    import torch
    shape = (12, 5, 4)
    x = generic(shape, seed=12)
    x[0, 0, 3] = np.nan
    wq, wnan = quantile_ref.quantile(x, P3)
    t = torch.from_numpy(x).cuda()
    q, nan = _raw_call(t.data_ptr(), shape, P3, want_nan=False)
    assert same_bits(q, wq) and (nan == -7).all()
    q, nan = _raw_call(t.data_ptr(), shape, P3, want_q=False)
    assert (q == -7.0).all() and same_bits(nan.astype(np.uint64), wnan)


def test_trace_aligned_to_8_bytes_only():
    """an even dim whose trace starts 8 bytes off a 16-byte boundary (the raw ABI; torch's own allocations never do): 8-byte lanes"""
    import torch
    shape = (30, 7, 12)
    x = generic(shape, seed=21)
    buf = torch.empty(x.size + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:] = torch.from_numpy(x.ravel()).cuda()
    q, nan = _raw_call(buf.data_ptr() + 8, shape, PROBS["sixteen"])
    wq, wnan = quantile_ref.quantile(x, PROBS["sixteen"])
    assert same_bits(q, wq) and same_bits(nan.astype(np.uint64), wnan)


def test_same_input_twice_gives_the_same_bits():
    x = hard_columns(64, 20, seed=31)
    a, b = N.quantile_draws(x, P16), N.quantile_draws(x, P16)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert_equals_ref(x, P16, got=a)


def test_tensor_and_array_inputs_agree():
    import torch
    x = generic((30, 9, 8), seed=2)
    a = N.quantile_draws(x, P3)
    t = torch.from_numpy(x).cuda()
    b = N.quantile_draws(t, P3)
    c = N.quantile_draws(torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda().permute(1, 0, 2), np.array(P3))   # not contiguous
    assert a[0].shape == (3, 8) and a[1].shape == (8,)
    for g in (b, c):
        assert same_bits(a[0], g[0]) and same_bits(a[1], g[1])
    assert (t.cpu().numpy() == x).all()                            # read where it lies, unchanged
    assert_equals_ref(x, P3, got=a)
    with pytest.raises(N.NutsAmdError, match="nm_quantile_draws"):
        N.quantile_draws(t, [0.5, 1.5])


def _warm_batch(chains, tune, seed):
    b = N.ChainBatch(N.DiagNutsSettings(num_chains=chains, seed=seed, num_tune=tune), N.LogpSpec.iid_normal(3, 1.0), chains)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    b.draw_device(tune)
    return b


@pytest.fixture(scope="module")
def three_runs():
    """the same seed three times: draw_summary with quantiles, draw_summary as the parent's signature has it, the draws themselves"""
    b = _warm_batch(64, 100, seed=23)
    with_q, st_q = b.draw_summary(50, quantiles=P3)
    b.close()
    b = _warm_batch(64, 100, seed=23)
    plain, st_plain = b.draw_summary(50, False, True, 32)
    b.close()
    b = _warm_batch(64, 100, seed=23)
    pos, st = b.draw_many(50)
    b.close()
    return with_q, st_q, plain, st_plain, pos, st


def test_draw_summary_with_quantiles(three_runs):
    with_q, st_q, _, _, pos, st = three_runs
    assert st_q.tobytes() == st.tobytes()
    want, wnan = quantile_ref.quantile(pos, P3)
    assert (wnan == 0).all() and same_bits(with_q.quantiles, want) and with_q.quantile_probs.tolist() == P3
    assert with_q.quantiles.shape == (3, 3) and (np.diff(with_q.quantiles, axis=0) > 0).all()
    # iid normal around 1.0 with unit sd: 1 - 1.645, 1, 1 + 1.645 (3200 draws: the 5 % point's standard error is 0.04)
    assert (np.abs(with_q.quantiles - np.array([[-0.645], [1.0], [2.645]])) < 0.2).all()


def test_draw_summary_without_quantiles_is_the_parents(three_runs):
    import dataclasses
    with_q, _, plain, st_plain, _, st = three_runs
    assert plain.quantiles is None and plain.quantile_probs is None and st_plain.tobytes() == st.tobytes()
    names = [f.name for f in dataclasses.fields(N.Summary)]
    assert names[-2:] == ["quantiles", "quantile_probs"] and len(names) == 13
    for name in names[:-2]:                                        # and asking for quantiles changes none of the parent's fields
        a, b = getattr(plain, name), getattr(with_q, name)
        assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b, name
