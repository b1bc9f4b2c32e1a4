"""Expanded draws on the device (`CpuLogpFunc::expand_vector`, reference src/math/cpu_math.rs:892-899; `Chain::expanded_draw`,
src/chain.rs:190-204): nm_engine_expand on hand-made rows and d_expanded of the draw calls against the expansion computed here with
numpy, operation by operation — the exponential is the oracle's restatement of the device's (nmo_scalar_fn op 0, bit-equal to the device
function: tests/test_gpu_units.py), the products and sums are single IEEE operations (the units are built without contraction).

Every comparison is bit for bit.  The one allowance is helpers.assert_bit_exact's: where BOTH sides are NaN the payloads are not compared
(which NaN an arithmetic operation returns for a NaN or invalid operand is the processor's choice, x86 and gfx950 choose differently);
a NaN that only passes through the exponential keeps its bits on both sides and a NaN on one side only is a mismatch."""
import ctypes as C

import numpy as np
import pytest

import nuts_rs_amd as N
from test_expand_abi import expanding_module

pytestmark = pytest.mark.gpu

SPECIALS = [0.0, -0.0, 709.9, -745.2, np.nan, np.inf, -np.inf, 1.0, -1.0, 5e-324, 709.782712893384, -708.4]


def oexp(oracle, a):
    """exp of every element in the engine's arithmetic (the oracle's scalar entry point)."""
    L, cfg = oracle.lib(), oracle.gpu_cfg(64)
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return np.array([L.nmo_scalar_fn(C.byref(cfg), 0, float(v), 0.0) for v in flat]).reshape(np.shape(a))


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~both_nan)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def eight_schools_expansion(oracle, pos):
    """(mu, log tau, theta~[8]) -> (mu, tau, theta[8]): tau = exp(log tau), theta_i = mu + tau * theta~_i as a product and a sum."""
    out = np.empty(pos.shape)
    with np.errstate(all="ignore"):
        tau = oexp(oracle, pos[..., 1])
        out[..., 0] = pos[..., 0]
        out[..., 1] = tau
        prod = tau[..., None] * pos[..., 2:]
        out[..., 2:] = pos[..., 0][..., None] + prod
    return out


def module_expansion(oracle, pos):
    """tests/user_density/my_expanding_normal.hpp: exp of every element, then x_0 * x_{dim-1}."""
    with np.errstate(all="ignore"):
        return np.concatenate([oexp(oracle, pos), (pos[..., 0] * pos[..., -1])[..., None]], axis=-1)


def rows_with_specials(n_rows, dim, seed):
    """Random rows; the special values walk through the columns of the first rows (every row keeps ordinary neighbours)."""
    x = np.random.default_rng(seed).normal(0.0, 2.0, (n_rows, dim))
    for k, v in enumerate(SPECIALS):
        x[k % n_rows, (k // n_rows + k) % dim] = v
    for k, v in enumerate(SPECIALS[:max(n_rows - 1, 0)]):
        x[n_rows - 1 - k, min(1, dim - 1)] = v      # ... and through column 1 (8 schools: log tau) of the last rows
    if n_rows > 2 * len(SPECIALS):
        x[len(SPECIALS), :] = np.nan                # a failed chain's row on the host path
    return x


def small_settings(chains, tune=20, draws=30, seed=31):
    return N.DiagNutsSettings(num_chains=chains, seed=seed, num_tune=tune, num_draws=draws)


# ---- nm_engine_expand on hand-made rows --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schools_batch():
    # a grid of 2 blocks: 1025 rows are 3 tiles of 409 rows, more than one pass of the grid
    b = N.ChainBatch(small_settings(4), N.LogpSpec.eight_schools(), 4, grid_blocks=2)
    yield b
    b.close()


@pytest.mark.parametrize("n_rows", [1, 3, 67, 1025])
def test_expand_eight_schools_rows(oracle, schools_batch, n_rows):
    assert schools_batch.expanded_dim() == 10
    x = rows_with_specials(n_rows, 10, seed=n_rows)
    same_bits(schools_batch.expand(x), eight_schools_expansion(oracle, x), f"8 schools, {n_rows} rows")


def test_expand_takes_device_tensors_and_leading_axes(oracle, schools_batch):
    import torch
    x = rows_with_specials(6 * 7, 10, seed=5).reshape(6, 7, 10)
    got = schools_batch.expand(torch.from_numpy(x).cuda())
    assert got.is_cuda and tuple(got.shape) == (6, 7, 10)
    same_bits(got.cpu().numpy(), eight_schools_expansion(oracle, x), "device tensor")
    # an odd element offset: neither the rows nor the outputs start on a 16-byte boundary
    buf = torch.from_numpy(np.concatenate([[0.0], x.reshape(-1)])).cuda()
    same_bits(schools_batch.expand(buf[1:].view(42, 10)).cpu().numpy(), eight_schools_expansion(oracle, x.reshape(42, 10)), "odd offset")


@pytest.mark.parametrize("n_rows,dim", [(1, 1), (5, 2), (67, 33), (130, 128)])
def test_expand_module_rows(oracle, n_rows, dim):
    """edim = dim + 1 != dim, odd dims (rows off the 16-byte grid), the last element reads both ends of its row."""
    b = N.ChainBatch(small_settings(2), N.LogpSpec.module(dim, expanding_module(dim), np.ones(dim)), 2)
    try:
        assert b.expanded_dim() == dim + 1
        x = rows_with_specials(n_rows, dim, seed=100 + dim)
        same_bits(b.expand(x), module_expansion(oracle, x), f"module, {n_rows} x {dim}")
    finally:
        b.close()


@pytest.mark.parametrize("n_rows,dim", [(2, 2049), (3, 2100)])
def test_expand_module_rows_longer_than_the_tile(oracle, n_rows, dim):
    """Rows that do not fit the kernel's LDS tile (2048 doubles): the functor reads global memory, a block takes 1024 outputs of a row
    at a time — three chunks per row here, the last one ragged, more (row, chunk) items than the grid of 2 blocks has blocks."""
    b = N.ChainBatch(small_settings(2), N.LogpSpec.module(dim, expanding_module(dim), np.ones(dim)), 2, grid_blocks=2)
    try:
        assert b.expanded_dim() == dim + 1
        x = rows_with_specials(n_rows, dim, seed=dim)
        same_bits(b.expand(x), module_expansion(oracle, x), f"module, {n_rows} x {dim}")
    finally:
        b.close()


def test_expand_identity_is_a_copy():
    b = N.ChainBatch(small_settings(2), N.LogpSpec.iid_normal(5), 2)
    try:
        assert b.expanded_dim() == 5
        x = rows_with_specials(3, 5, seed=9)
        got = b.expand(x)
        assert (got.view(np.uint64) == x.view(np.uint64)).all()          # a copy keeps every NaN's bits
        launches = b.counters()["kernel_launches"]
        import torch
        t = torch.from_numpy(x).cuda()
        N._lib.check(N.load_library().nm_engine_expand(b._h, 3, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr())))    # in place: a no-op
        b.synchronize()
        assert (t.cpu().numpy().view(np.uint64) == x.view(np.uint64)).all() and b.counters()["kernel_launches"] == launches
    finally:
        b.close()


def test_expand_identity_wide_chain():
    """A row longer than the kernel's LDS tile, through an engine whose chain spans two blocks."""
    b = N.ChainBatch(small_settings(1), N.LogpSpec.iid_normal(4097), 1)
    try:
        assert b.blocks_per_chain() == 2 and b.expanded_dim() == 4097
        x = rows_with_specials(2, 4097, seed=11)
        assert (b.expand(x).view(np.uint64) == x.view(np.uint64)).all()
    finally:
        b.close()


# ---- the draw calls ----------------------------------------------------------------------------------------------------------
FAMILIES = {"wave": dict(), "group": dict(lane_groups=2), "lane": dict(lane_chains=2)}
CHAINS, TUNE, DRAWS = 70, 20, 30


def schools_run(kw):
    b = N.ChainBatch(small_settings(CHAINS, TUNE, DRAWS), N.LogpSpec.eight_schools(), CHAINS, **kw)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    return b


def family_of(b):
    return "lane" if b.lane_launches() else "group" if b.group_launches() else "wave"


@pytest.fixture(scope="module")
def plain_runs():
    """The runs that never ask for an expansion, one per kernel family: what the expanded runs must reproduce."""
    out = {}
    for name, kw in FAMILIES.items():
        b = schools_run(kw)
        pos, st, _ = b.expanded_draw_many(DRAWS)
        assert family_of(b) == name
        b.close()
        out[name] = (pos, st)
    return out


@pytest.mark.parametrize("family", list(FAMILIES))
def test_draws_with_expansion_eight_schools(oracle, plain_runs, family):
    pos0, st0 = plain_runs[family]
    b = schools_run(FAMILIES[family])
    try:
        res = b.expanded_draw_many(DRAWS, expanded=True)
        assert len(res) == 4 and family_of(b) == family
        pos, st, vec, ex = res
    finally:
        b.close()
    assert ex.shape == (DRAWS, CHAINS, 10) and (st["chain_status"] == 0).all()
    same_bits(ex, eight_schools_expansion(oracle, pos), f"{family}: expanded == f(positions)")
    # the expansion changed nothing else: the chains' random streams were never touched
    assert (pos.view(np.uint64) == pos0.view(np.uint64)).all(), "positions moved"
    assert st.tobytes() == st0.tobytes(), "statistics moved"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_device_buffers_two_calls_eight_schools(oracle, plain_runs, family):
    import torch
    pos0, st0 = plain_runs[family]
    d_pos = torch.full((DRAWS, CHAINS, 10), float("nan"), dtype=torch.float64, device="cuda")
    d_ex = torch.full((DRAWS, CHAINS, 10), float("nan"), dtype=torch.float64, device="cuda")
    d_st = torch.zeros((DRAWS, CHAINS, N.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = schools_run(FAMILIES[family])
    try:
        half = DRAWS // 2
        for lo in (0, half):                        # the second call's rows follow the first's
            b.draw_device_ex(half, positions=d_pos[lo:].data_ptr(), stats=d_st[lo:].data_ptr(), expanded=d_ex[lo:].data_ptr())
        assert family_of(b) == family
    finally:
        b.close()
    pos, ex = d_pos.cpu().numpy(), d_ex.cpu().numpy()
    st = d_st.cpu().numpy().reshape(-1).view(N.STATS_DTYPE).reshape(DRAWS, CHAINS)
    assert (pos.view(np.uint64) == pos0.view(np.uint64)).all() and st.tobytes() == st0.tobytes()
    same_bits(ex, eight_schools_expansion(oracle, pos0), f"{family}: device buffers, two calls")


def test_draws_with_expansion_module(oracle):
    dim = 33
    prec = np.exp(np.random.default_rng(3).uniform(-1, 1, dim))
    b = N.ChainBatch(small_settings(5, 10, 10), N.LogpSpec.module(dim, expanding_module(dim), prec), 5)
    try:
        assert (b.set_position(b.init_positions_uniform()) == 0).all()
        pos, st, _, ex = b.expanded_draw_many(20, expanded=True)
    finally:
        b.close()
    assert ex.shape == (20, 5, dim + 1) and (st["chain_status"] == 0).all()
    same_bits(ex[..., :dim], oexp(oracle, pos), "module: exp(positions)")
    same_bits(ex[..., dim], pos[..., 0] * pos[..., dim - 1], "module: the product of the row's ends")


def test_draws_with_expansion_identity():
    runs = []
    for expanded in (True, False):
        b = N.ChainBatch(small_settings(6, 10, 10), N.LogpSpec.iid_normal(5), 6)
        try:
            assert b.expanded_dim() == 5 and (b.set_position(b.init_positions_uniform()) == 0).all()
            runs.append(b.expanded_draw_many(20, expanded=expanded))
        finally:
            b.close()
    pos, st, _, ex = runs[0]
    assert (ex.view(np.uint64) == pos.view(np.uint64)).all()
    assert (pos.view(np.uint64) == runs[1][0].view(np.uint64)).all() and st.tobytes() == runs[1][1].tobytes()


def test_sample_returns_the_expanded_trace(oracle):
    s = small_settings(3, 10, 5)
    pos, st, ex = N.sample(s, N.LogpSpec.eight_schools(), expanded=True)
    pos0, st0 = N.sample(s, N.LogpSpec.eight_schools())
    assert (pos.view(np.uint64) == pos0.view(np.uint64)).all() and st.tobytes() == st0.tobytes()
    same_bits(ex, eight_schools_expansion(oracle, pos), "sample(expanded=True)")


def test_argument_errors_launch_nothing():
    import torch
    b = schools_run({})
    try:
        buf = torch.zeros(2 * 5 * CHAINS * 10, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        before = b.counters()
        with pytest.raises(N.NutsAmdError) as e:                 # an expansion has nothing to expand without the positions
            b.draw_device_ex(5, expanded=buf.data_ptr())
        assert e.value.status == 1
        with pytest.raises(N.NutsAmdError) as e:                 # in place: only the identity may
            b.draw_device_ex(5, positions=buf.data_ptr(), expanded=buf.data_ptr())
        assert e.value.status == 1
        with pytest.raises(N.NutsAmdError) as e:                 # a partial overlap
            b.draw_device_ex(5, positions=buf.data_ptr(), expanded=buf[5 * CHAINS * 10 - 8:].data_ptr())
        assert e.value.status == 1
        with pytest.raises(N.NutsAmdError) as e:
            N._lib.check(N.load_library().nm_engine_expand(b._h, 7, C.c_void_p(buf.data_ptr()), C.c_void_p(buf[8:].data_ptr())))
        assert e.value.status == 1
        after = b.counters()
        assert after["kernel_launches"] == before["kernel_launches"] and after["total_draws"] == before["total_draws"]
        # the engine is as it was: the next call draws what a fresh engine draws
        pos, st, _ = b.expanded_draw_many(3)
    finally:
        b.close()
    b2 = schools_run({})
    try:
        pos2, st2, _ = b2.expanded_draw_many(3)
    finally:
        b2.close()
    assert (pos.view(np.uint64) == pos2.view(np.uint64)).all() and st.tobytes() == st2.tobytes()
