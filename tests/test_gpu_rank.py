"""nm_transform_draws on the GPU (csrc/rank_transform.hip): rank2, the NaN counts and the indicator equal the numpy restatement of the
definition (tests/rank_ref.py) BIT FOR BIT, the scores equal the host twin nm_rank_normal_score applied to the restated rank2 — on the
smallest shapes that cross each boundary of the kernels (one key, one past a wavefront, more than one slab and ragged, 8- and 16-byte
lanes, a misaligned base, ragged column batches, selected chains, the middle draw of an odd split trace), and on columns built so that
single passes of the sort reorder nothing or everything.  Then the front ends: rank_diagnostics and draw_summary(rank_normalized=True)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib

import rank_ref

pytestmark = pytest.mark.gpu

S = N.NM_RANK_SLAB_KEYS


def generic(shape, seed):
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


def assert_equals_ref(x, kind=0, param=None, split=True, chain_ids=None, max_scratch_bytes=0, got=None):
    if got is None:
        got = N.transform_draws(x, kind, param, split=split, chain_ids=chain_ids, ranks=kind != 2, max_scratch_bytes=max_scratch_bytes)
    out, r2, nan = got
    wout, wr2, wnan = rank_ref.transform(x, kind, param, split, chain_ids)
    assert same_bits(nan, wnan), f"nan_count: {nan} vs {wnan}"
    if kind != 2:
        assert r2.dtype == np.uint32 and r2.shape == wr2.shape
        bad = np.argwhere(r2 != wr2)
        assert len(bad) == 0, f"rank2 differs at {len(bad)} places, first [draw, chain, column] {bad[:4].tolist()}: {[(int(r2[tuple(i)]), int(wr2[tuple(i)])) for i in bad[:4]]}"
    else:
        assert r2 is None
    assert same_bits(out, wout), "the scores differ from the host twin's" if kind != 2 else "the indicator differs"
    return got


SHAPES = [
    ((1, 1, 1), False),          # one key
    ((2, 1, 1), True),
    ((2, 1, 1), False),
    ((4, 1, 1), True),
    ((5, 2, 3), True),           # odd N, split: the middle draw is outside the pool
    ((5, 2, 3), False),
    ((7, 9, 3), False),          # 63 keys, odd dim: 8-byte lanes
    ((7, 9, 3), True),
    ((13, 5, 1), False),         # 65 keys: one past a wavefront
    ((50, 64, 10), True),        # K4's row: 16-byte lanes, several rows per wavefront
    ((2 * S + 37, 1, 3), False),          # more than one slab, the last one ragged
    ((S // 4 + 1, 4, 18), True),          # every wavefront of a block, a ragged column tile
]


@pytest.mark.parametrize("shape,split", SHAPES, ids=["x".join(map(str, s)) + ("-split" if sp else "") for s, sp in SHAPES])
def test_device_equals_restatement(shape, split):
    x = generic(shape, seed=sum(shape))
    assert_equals_ref(x, 0, None, split)
    c = x[0, 0].copy()                                          # a centre equal to an element of every column
    assert_equals_ref(x, 1, c, split)
    assert_equals_ref(x, 2, c, split)


def hard_columns(n_draws, n_chains, seed):
    """one column per way a pass of the sort can have nothing to reorder, or everything, between generic columns"""
    rng = np.random.default_rng(seed)
    n = n_draws * n_chains
    x = generic((n_draws, n_chains, 15), seed).reshape(n, 15)
    x[:, 1] = -3.75                                                                   # all equal: every pass is the identity
    x[:, 2] = np.where(rng.random(n) < 0.3, 1.0, -2.0)                                # two values
    base = np.float64(1.2345678).view(np.uint64) & ~np.uint64(0xFF)
    x[:, 3] = (base | rng.integers(0, 256, size=n).astype(np.uint64)).view(np.float64)          # only the last byte differs: the first pass decides
    mant = np.uint64(0x000F_1234_5678_9ABC)
    x[:, 4] = ((rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(56)) | mant).view(np.float64)   # only the top byte and the sign differ
    x[:, 5] = rng.choice([-1e-3, -0.0, 0.0, 1e-3, -5e-324, 5e-324], size=n)           # both zeros
    x[:, 6] = rng.choice([-np.inf, np.inf, -1.0, 0.5, 2.0], size=n)
    x[:, 7] = rng.integers(-40, 40, size=n) * 5e-324                                  # subnormals of both signs
    x[:, 8] = rng.integers(0, 4, size=n).astype(np.float64)                           # heavy ties
    x[:, 9] = rng.permutation(n).astype(np.float64)                                   # every pass reorders
    x[:, 10] = np.arange(n) * 0.37 - 11.0                                             # ascending
    x[:, 11] = -np.arange(n) * 1e-200                                                 # descending
    x[:, 12] = rng.normal(size=n)
    x[rng.integers(0, n, size=3), 12] = np.nan                                        # a NaN column between clean ones
    x[7, 12], x[n - 5, 12] = -np.nan, np.nan                                          # (two that are in the pool of the split trace as well)
    return x.reshape(n_draws, n_chains, 15)


@pytest.fixture(scope="module")
def hard():
    return hard_columns((S + 1500) // 4, 4, seed=5)                                   # two slabs, the second ragged, all four wavefronts


@pytest.mark.parametrize("split", [False, True])
def test_columns_that_defeat_single_passes(hard, split):
    _, _, nan = assert_equals_ref(hard, 0, None, split)
    assert nan[12] >= 2 and nan.sum() == nan[12]


def test_folded_and_indicator_on_hard_columns(hard):
    c = np.array([0.0, -3.75, -0.5, 1.2345678, 0.0, 0.0, 0.5, 0.0, 1.5, 1000.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    c[0], c[13] = hard[3, 1, 0], hard[0, 0, 13]                 # centres equal to an element; 1.5 and -0.5: symmetric pairs tie exactly
    assert_equals_ref(hard, 1, c, True)
    t = c.copy()
    t[5], t[8], t[14] = -0.0, 2.0, np.nan                       # -0.0 against both zeros; a threshold equal to elements; a NaN threshold
    out, _, nan = assert_equals_ref(hard, 2, t, True)
    assert np.isnan(out[:, :, 14]).all() and nan[14] == 0 and nan[12] >= 2 and np.isnan(out[:, :, 12]).sum() == nan[12]


def test_misaligned_base_takes_the_narrow_lanes():
    import torch
    x = generic((33, 5, 4), seed=9)
    flat = torch.zeros(x.size + 1, dtype=torch.float64, device="cuda")
    view = flat[1:].view(33, 5, 4)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    wide = N.transform_draws(torch.from_numpy(x).cuda(), 0, ranks=True)
    narrow = N.transform_draws(view, 0, ranks=True)
    assert same_bits(wide[0].cpu().numpy(), narrow[0].cpu().numpy()) and same_bits(wide[1].cpu().numpy(), narrow[1].cpu().numpy())
    assert_equals_ref(x, 0, got=(narrow[0].cpu().numpy(), narrow[1].cpu().numpy(), narrow[2]))


@pytest.mark.parametrize("dim", [5, 6])
def test_column_batches_do_not_change_the_bits(dim):
    x = generic((40, 3, dim), seed=dim)
    n = 40 * 3
    two_columns = 2 * (24 * n + 1024 * -(-n // S)) + 100        # the header's scratch per column: three batches, for dim 5 the last one ragged
    whole = assert_equals_ref(x, 0)
    batched = assert_equals_ref(x, 0, max_scratch_bytes=two_columns)
    assert_equals_ref(x, 1, x[1, 1], max_scratch_bytes=1)       # never fewer than one column
    assert same_bits(whole[0], batched[0]) and same_bits(whole[1], batched[1])


def test_selected_chains():
    x = generic((21, 7, 4), seed=3)
    x[4, 1, 2] = np.nan                                         # in a chain that is left out: not counted
    for kind in (0, 1, 2):
        out, _, nan = assert_equals_ref(x, kind, x[0, 2], True, chain_ids=[0, 2, 5])
        assert out.shape == (21, 3, 4) and (nan == 0).all()


def _raw(t, kind, split, out, r2, nan, param=None):
    import torch
    n_draws, n_chains, dim = t.shape
    spec = _lib.NmTransformSpec(n_draws, n_chains, dim, kind, int(split), 0, None, 0)
    o = _lib.NmTransformOutputs(*(None if b is None else b.data_ptr() for b in (out, r2, nan)))
    torch.cuda.synchronize()
    L = N.load_library()
    st = L.nm_transform_draws(C.byref(spec), C.c_void_p(t.data_ptr()), C.c_void_p(None if param is None else param.data_ptr()), C.byref(o), None)
    torch.cuda.synchronize()
    return st


def test_each_output_absent_in_turn_and_twice_the_same():
    import torch
    x = generic((31, 6, 4), seed=17)
    x[3, 3, 1] = np.nan
    t = torch.from_numpy(x).cuda()
    full = assert_equals_ref(x, 0)
    again = N.transform_draws(x, 0, ranks=True)
    assert all(same_bits(a, b) for a, b in zip(full, again))
    as_tensor = N.transform_draws(t, 0, ranks=True)             # tensor against array input
    assert isinstance(as_tensor[0], torch.Tensor) and as_tensor[0].is_cuda and as_tensor[1].dtype == torch.uint32
    assert same_bits(as_tensor[0].cpu().numpy(), full[0]) and same_bits(as_tensor[1].cpu().numpy(), full[1]) and same_bits(as_tensor[2], full[2])
    mine = torch.empty((31, 6, 4), dtype=torch.float64, device="cuda")
    given = N.transform_draws(t, 0, out=mine)
    assert given[0] is mine and given[1] is None and same_bits(mine.cpu().numpy(), full[0])
    none, r2, nan = N.transform_draws(x, 0, out=False, ranks=True)
    assert none is None and same_bits(r2, full[1]) and same_bits(nan, full[2])
    out = torch.full((31, 6, 4), 7.0, dtype=torch.float64, device="cuda")
    r2 = torch.full((31, 6, 4), 7, dtype=torch.int32, device="cuda")
    assert _raw(t, 0, True, out, r2, None) == 0                  # no NaN counts
    assert same_bits(out.cpu().numpy(), full[0]) and same_bits(r2.cpu().numpy().view(np.uint32), full[1])
    c = torch.from_numpy(x[0, 0].copy()).cuda()
    out.fill_(7.0)
    assert _raw(t, 2, True, out, None, None, c) == 0
    assert same_bits(out.cpu().numpy(), rank_ref.transform(x, 2, x[0, 0])[0])


@pytest.mark.parametrize("shape,split,ids", [((60, 6, 4), True, None), ((61, 6, 4), True, [0, 2, 5]), ((40, 5, 3), False, None)],
                         ids=["60x6x4", "61x6x4-ids", "40x5x3-unsplit"])
def test_rank_diagnostics_equals_the_composition_of_the_restatements(shape, split, ids):
    rng = np.random.default_rng(shape[0])
    x = generic(shape, seed=shape[0])
    x[:, -1, 0] *= 3.0                                          # a chain of another scale
    x[:, :, 1] = rng.standard_cauchy(shape[:2])
    for t in range(1, shape[0]):                                # an autocorrelated column
        x[t, :, 2] = 0.7 * x[t - 1, :, 2] + rng.normal(size=shape[1])
    got = N.rank_diagnostics(x, split=split, max_lag=16, chain_ids=ids)
    want = rank_ref.rank_diagnostics(x, split, 16, ids)
    for name in rank_ref.DIAG_FIELDS:
        assert same_bits(getattr(got, name), getattr(want, name)), name
    import torch
    on_device = N.rank_diagnostics(torch.from_numpy(x).cuda(), split=split, max_lag=16, chain_ids=ids)
    for name in rank_ref.DIAG_FIELDS:
        assert same_bits(getattr(on_device, name), getattr(got, name)), name


def _warm_batch(chains, tune, seed):
    b = N.ChainBatch(N.DiagNutsSettings(num_chains=chains, seed=seed, num_tune=tune), N.LogpSpec.iid_normal(3, 1.0), chains)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    b.draw_device(tune)
    return b


@pytest.fixture(scope="module")
def three_runs():
    """the same seed three times: draw_summary with the rank diagnostics, draw_summary as the parent's signature has it, the draws themselves"""
    b = _warm_batch(64, 100, seed=23)
    ranked, st_r = b.draw_summary(50, rank_normalized=True)
    b.close()
    b = _warm_batch(64, 100, seed=23)
    plain, st_plain = b.draw_summary(50, False, True, 32, None)
    b.close()
    b = _warm_batch(64, 100, seed=23)
    pos, st = b.draw_many(50)
    b.close()
    return ranked, st_r, plain, st_plain, pos, st


def test_draw_summary_rank_normalized(three_runs):
    ranked, st_r, _, _, pos, st = three_runs
    assert st_r.tobytes() == st.tobytes() and isinstance(ranked, N.RankSummary) and isinstance(ranked, N.Summary)
    want = N.rank_diagnostics(pos, split=True, max_lag=32)
    for name in ("rhat_rank", "ess_bulk", "ess_tail", "ess_bulk_truncated", "ess_tail_truncated"):
        assert same_bits(getattr(ranked, name), getattr(want, name)), name
    assert (want.nan_count == 0).all() and (ranked.rhat_rank < 1.05).all() and (ranked.ess_bulk > 200).all() and (ranked.ess_tail > 200).all()
    names = [f.name for f in dataclasses.fields(N.RankSummary)]
    assert names[:13] == [f.name for f in dataclasses.fields(N.Summary)]
    assert names[13:] == ["rhat_rank", "ess_bulk", "ess_tail", "ess_bulk_truncated", "ess_tail_truncated"]


def test_draw_summary_by_default_is_the_parents(three_runs):
    ranked, _, plain, st_plain, _, st = three_runs
    assert type(plain) is N.Summary and st_plain.tobytes() == st.tobytes()
    for name in ("rhat_rank", "ess_bulk", "ess_tail", "ess_bulk_truncated", "ess_tail_truncated"):
        assert getattr(plain, name) is None
    for f in dataclasses.fields(N.Summary):                      # asking for the rank diagnostics changes none of the parent's fields
        a, b = getattr(plain, f.name), getattr(ranked, f.name)
        assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b, f.name
