"""nm_stats_columns and nm_diagnose_stats on the GPU (csrc/stats_diag.hip): every output equals the numpy restatement of the definitions
(tests/diag_ref.py) BIT FOR BIT — the floating outputs through their uint64 view, a NaN included — on records synthesised in numpy, at
the smallest shapes that cross each boundary of the kernels (one record, one short of and one past a 64-chain run, more than one block,
one chain past a pooled chunk, many blocks) and in each of the three phases.  Then the events (order, capacity, guard), absent outputs,
a misaligned base, the composition with summarize_draws, and one engine run through draw_summary."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib
from nuts_rs_amd.sampler import DIAG_CHAIN_COUNTS, DIAG_CHAIN_VALUES, DIAG_POOLED_COUNTS, DIAG_POOLED_VALUES

import diag_ref
import summary_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 63), (3, 65), (7, 130), (40, 33), (5, 2049)]
PHASES = ["all", "sampling", "tuning"]
GUARD = 0x5A5A5A5A5A5A5A5A
ITEM = N.STATS_DTYPE.itemsize


def synth(n_draws, n_chains, seed=None):
    """records with everything the definitions distinguish: tuning then sampling rows, dense divergences, depths up to 40, n_steps near
    2^63 (the sums wrap), and — where the shape has the chains — an unwritten tail, a chain unwritten throughout, a chain that ends with
    status 2, a NaN energy, an infinite energy, a constant energy; the same specials again in the last 64-chain run"""
    rng = np.random.default_rng(1000 * n_draws + n_chains if seed is None else seed)
    shape = (n_draws, n_chains)
    st = np.zeros(shape, dtype=N.STATS_DTYPE)
    st["draw"] = np.arange(n_draws, dtype=np.uint64)[:, None]
    st["chain"] = np.arange(n_chains, dtype=np.uint64)[None, :]
    st["depth"] = rng.integers(0, 41, size=shape)
    st["maxdepth_reached"] = st["depth"] >= 10
    st["diverging"] = (rng.random(shape) < 0.3) * rng.integers(1, 3, size=shape)
    st["tuning"] = (np.arange(n_draws)[:, None] < rng.integers(0, n_draws // 2 + 1, size=n_chains)[None, :]) * 1
    st["n_steps"] = np.where(rng.random(shape) < 0.5, rng.integers(2**63 - 1000, 2**63, size=shape, dtype=np.uint64), rng.integers(1, 1024, size=shape, dtype=np.uint64))
    st["index_in_trajectory"] = rng.integers(-500, 500, size=shape)
    st["transformation_index"] = rng.integers(-2**62, 2**62, size=shape)
    st["transformation_update_id"] = rng.integers(-1, 5, size=shape)
    st["num_eigenvalues"] = rng.integers(0, 2**64, size=shape, dtype=np.uint64)          # (conversions that round)
    for name in ("step_size", "step_size_bar", "mean_tree_accept", "mean_tree_accept_sym", "max_energy_error", "logp", "energy_error",
                 "fisher_distance", "divergence_energy_error", "energy_change", "average_step_size"):
        st[name] = rng.normal(size=shape) * np.exp(rng.uniform(-3, 3))
    st["mean_tree_accept"] = rng.uniform(0, 1, size=shape)
    st["divergence_energy_error"][st["diverging"] == 0] = np.nan
    st["energy"] = 50.0 + np.cumsum(rng.normal(size=shape), axis=0) * 0.5 + rng.normal(size=shape)
    raw = st.view(np.uint8).reshape(n_draws, n_chains, ITEM)
    for base in sorted({0, 64 * ((n_chains - 1) // 64)}):
        c = [base + i for i in range(1, 7)]
        if c[0] < n_chains:
            raw[n_draws // 2:, c[0]] = 0xFF                       # stopped half way: an unwritten tail
        if c[1] < n_chains:
            raw[:, c[1]] = 0xFF                                   # never started
        if c[2] < n_chains:
            st["chain_status"][n_draws - 1, c[2]] = 2             # its last row says LOGP_FATAL
        if c[3] < n_chains:
            st["energy"][min(1, n_draws - 1), c[3]] = np.nan
        if c[4] < n_chains:
            st["energy"][n_draws - 1, c[4]] = np.inf
        if c[5] < n_chains:
            st["energy"][:, c[5]] = -12.5                         # v = 0
    return st


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def raw_diagnose(t, n_draws, n_chains, phase=0, max_events=64, threshold=0.3, absent=(), guard_rows=8):
    """nm_diagnose_stats on the tensor t with every output but `absent`: {name: host array}; the events buffer is guard_rows longer than
    its capacity and pre-filled, so that a write beyond the capacity shows"""
    import torch
    dev = t.device
    bufs = dict(chain_counts=torch.full((n_chains, 6), GUARD, dtype=torch.int64, device=dev), chain_values=torch.full((n_chains, 6), -7.0, dtype=torch.float64, device=dev),
                pooled_counts=torch.full((8,), GUARD, dtype=torch.int64, device=dev), pooled_values=torch.full((3,), -7.0, dtype=torch.float64, device=dev),
                depth_hist=torch.full((32,), GUARD, dtype=torch.int64, device=dev), events=torch.full((max_events + guard_rows, 2), GUARD, dtype=torch.int64, device=dev),
                n_events=torch.full((1,), GUARD, dtype=torch.int64, device=dev))
    out = _lib.NmDiagOutputs()
    for k, b in bufs.items():
        setattr(out, "d_" + k, None if k in absent else b.data_ptr())
    spec = _lib.NmDiagSpec(n_draws, n_chains, phase, 0 if "events" in absent else max_events, threshold)
    torch.cuda.synchronize()
    L = N.load_library()
    status = L.nm_diagnose_stats(C.byref(spec), C.c_void_p(t.data_ptr()), C.byref(out), None)
    torch.cuda.synchronize()
    assert status == 0, L.nm_diag_last_error()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


def assert_raw_equals_ref(got, want, max_events, absent=()):
    for k in ("chain_counts", "chain_values", "pooled_counts", "pooled_values", "depth_hist"):
        if k in absent:
            assert (u64(got[k]) == (GUARD if got[k].dtype == np.int64 else u64(np.float64(-7.0)))).all(), f"{k} was written although absent"
        else:
            bad = np.argwhere(u64(got[k]) != u64(getattr(want, k)))
            assert len(bad) == 0, f"{k} differs at {bad[:4].tolist()}: {[(got[k][tuple(i)], getattr(want, k)[tuple(i)]) for i in bad[:4]]}"
    if "n_events" not in absent:
        assert int(u64(got["n_events"])[0]) == want.n_events
    ev = u64(got["events"])
    kept = 0 if "events" in absent else min(want.n_events, max_events)
    assert (ev[:kept] == want.events[:kept]).all(), "events differ (order is (t, c))"
    assert (ev[kept:] == GUARD).all(), "something was written beyond the events"


def to_device(st):
    import torch
    return torch.from_numpy(st.view(np.uint8).reshape(st.shape + (ITEM,))).cuda()


@pytest.fixture(scope="module")
def cases():
    """per shape the records, once"""
    return {s: synth(*s) for s in SHAPES}


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_device_equals_restatement(cases, shape, phase):
    st = cases[shape]
    code = {"all": 0, "sampling": 1, "tuning": 2}[phase]
    want = diag_ref.diagnose(st, code, max_events=2**40, bfmi_threshold=0.9)
    got = raw_diagnose(to_device(st), *shape, phase=code, max_events=max(1, want.n_events + 3), threshold=0.9)          # larger than n_events
    assert_raw_equals_ref(got, want, want.n_events + 3)
    d = N.sampler_diagnostics(st, phase=phase, max_events=max(1, want.n_events // 2), bfmi_threshold=0.9)                 # the front end; smaller
    for i, k in enumerate(DIAG_CHAIN_COUNTS):
        assert (getattr(d, k) == want.chain_counts[:, i]).all(), k
    for i, k in enumerate(DIAG_CHAIN_VALUES):
        assert (u64(getattr(d, k)) == u64(want.chain_values[:, i])).all(), k
    for i, k in enumerate(DIAG_POOLED_COUNTS):
        assert getattr(d, "pooled_" + k) == int(want.pooled_counts[i]), k
    for i, k in enumerate(DIAG_POOLED_VALUES):
        assert u64(np.float64(getattr(d, "pooled_" + k))) == u64(want.pooled_values[i]), k
    kept = min(want.n_events, max(1, want.n_events // 2))
    assert d.n_events == want.n_events and d.events.shape == (kept, 2) and (d.events == want.events[:kept]).all() and (d.depth_hist == want.depth_hist).all()
    assert d.phase == phase


def test_the_synthetic_records_exercise_what_they_should(cases):
    st = cases[(7, 130)]
    want = diag_ref.diagnose(st, 0, max_events=2**40)
    cc, cv = want.chain_counts, want.chain_values
    assert cc[1, 0] == 3 and cc[1, 5] == 2**64 - 1 and cc[2, 0] == 0 and cc[3, 5] == 2 and cc[3, 0] == 7          # tail, never started, stopped
    assert np.isnan(cv[4, 3]) and np.isnan(cv[5, 3]) and cv[6, 2] == 0.0 and np.isnan(cv[6, 3])                  # NaN, inf, constant energy
    assert want.depth_hist[31] > 20 and st["depth"][st["chain_status"] != np.uint64(2**64 - 1)].max() == 40                                                  # the clip
    assert st["n_steps"][:, 0].astype(object).sum() >= 2**64 or st["n_steps"][:, 7].astype(object).sum() >= 2**64                                              # the sums wrap
    assert want.n_events > 64 * 3 and len(set(want.events[:, 1] // 64)) == 3                                      # events in every block, dense
    assert want.pooled_counts[0] == 130 - 4 and want.pooled_counts[7] >= 3                                        # chains 1, 2, 3 and 129 are not healthy
    sampling, tuning = diag_ref.diagnose(st, 1).pooled_counts[1], diag_ref.diagnose(st, 2).pooled_counts[1]
    assert sampling > 0 and tuning > 0 and sampling + tuning == want.pooled_counts[1]


@pytest.mark.parametrize("shape", [(7, 130), (33, 2049)], ids=["7x130", "33x2049"])
def test_events_capacity_order_and_guard(cases, shape):
    """33 x 2049: 33 x 33 = 1089 masks, more than the 1024 a block of the compaction owns — the events span blocks of every kernel"""
    st = cases[shape] if shape in cases else synth(*shape)
    want = diag_ref.diagnose(st, 0, max_events=2**40)
    assert want.n_events >= 200 and len(set((want.events[:, 1] // 64).tolist())) == -(-shape[1] // 64)          # dense: in every 64-chain run
    t = to_device(st)
    order = want.events[:, 0].astype(np.int64) * shape[1] + want.events[:, 1].astype(np.int64)
    assert (np.diff(order) > 0).all()                                           # the restatement's order IS lexicographic (t, c)
    for cap in (0, 1, want.n_events // 2, want.n_events, want.n_events + 5):
        if cap == 0:
            got = raw_diagnose(t, *shape, absent=("events",))                   # no capacity: d_events may be null, the count still comes
        else:
            got = raw_diagnose(t, *shape, max_events=cap)
        assert_raw_equals_ref(got, diag_ref.diagnose(st, 0, max_events=cap), cap, absent=("events",) if cap == 0 else ())


def test_each_output_absent_in_turn_and_twice_the_same(cases):
    shape = (7, 130)
    st, t = cases[shape], to_device(cases[shape])
    want = diag_ref.diagnose(st, 1, max_events=50, bfmi_threshold=0.5)
    first = raw_diagnose(t, *shape, phase=1, max_events=50, threshold=0.5)
    again = raw_diagnose(t, *shape, phase=1, max_events=50, threshold=0.5)
    assert_raw_equals_ref(first, want, 50)
    assert all((u64(first[k]) == u64(again[k])).all() for k in first)
    for name in ("chain_counts", "chain_values", "pooled_counts", "pooled_values", "depth_hist", "events", "n_events"):
        assert_raw_equals_ref(raw_diagnose(t, *shape, phase=1, max_events=50, threshold=0.5, absent=(name,)), want, 50, absent=(name,))
    only = raw_diagnose(t, *shape, phase=1, threshold=0.5, absent=("chain_counts", "chain_values", "pooled_counts", "depth_hist", "events", "n_events"))
    assert (u64(only["pooled_values"]) == u64(want.pooled_values)).all()


def misaligned(st):
    """the same records 8 bytes off a 16-byte boundary"""
    import torch
    nbytes = st.size * ITEM
    flat = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    view = flat[8:].view(st.shape + (ITEM,))
    view.copy_(to_device(st))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


def test_misaligned_base_gives_the_same_answers(cases):
    for shape in ((3, 65), (7, 130)):
        st = cases[shape]
        want = diag_ref.diagnose(st, 0, max_events=64)
        assert_raw_equals_ref(raw_diagnose(misaligned(st), *shape), want, 64)
        names = ["energy", "depth", "chain_status"]
        got = N.stats_columns(misaligned(st), names).cpu().numpy()
        assert (u64(got) == u64(diag_ref.stats_columns(st, names))).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (3, 65)], ids=["1", "63", "65x3"])
def test_columns_every_field(cases, shape):
    st = synth(*shape, seed=77) if shape not in cases else cases[shape]
    names = list(N.STATS_DTYPE.names)
    assert len(names) == N.NM_STAT_WORDS
    for fields in (names[::-1], names[:5] + ["energy", "energy"] + names[7:9], ["transformation_update_id"]):
        got = N.stats_columns(st, fields)
        assert got.is_cuda and tuple(got.shape) == shape + (len(fields),)
        got = got.cpu().numpy()
        assert (u64(got) == u64(diag_ref.stats_columns(st, fields))).all(), fields
        unwritten = st["chain_status"] == np.uint64(2**64 - 1)
        for i, f in enumerate(fields):                                          # the issue's statement of the same thing
            col = st[f].astype(np.float64)
            assert (u64(got[..., i])[~unwritten] == u64(col)[~unwritten]).all() and (u64(got[..., i])[unwritten] == 0x7FF8000000000000).all(), f
    with pytest.raises(ValueError):
        N.stats_columns(st, ["no_such_statistic"])
    with pytest.raises(N.NutsAmdError, match="nm_stats_columns"):
        N.stats_columns(st, [])


def test_columns_compose_with_summarize_draws():
    """the R-hat and ESS of lp__ and energy: summarize_draws over stats_columns equals the restatement over the same columns"""
    rng = np.random.default_rng(5)
    st = np.zeros((60, 6), dtype=N.STATS_DTYPE)
    for name in ("energy", "logp"):
        x = rng.normal(size=(60, 6))
        for t in range(1, 60):
            x[t] = 0.5 * x[t - 1] + x[t]
        st[name] = x
    cols = N.stats_columns(st, ["energy", "logp"])
    got = N.summarize_draws(cols, split=True, max_lag=16)
    want = summary_ref.summarize(np.stack([st["energy"], st["logp"]], axis=2), True, 16)
    for name in summary_ref.FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and (u64(a) == u64(b)).all(), name
    assert (got.ess > 20).all() and (got.rhat < 1.2).all()


def _funnel_batch(seed=31):
    b = N.ChainBatch(N.DiagNutsSettings(num_chains=128, seed=seed, num_tune=40), N.LogpSpec.funnel(11), 128)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    b.draw_device(40)
    return b


@pytest.fixture(scope="module")
def engine_runs():
    """the same seed three times: with the diagnostics, without the host statistics, as the parent's signature has it"""
    b = _funnel_batch()
    with_diag, st_diag = b.draw_summary(60, diagnostics=True)
    b.close()
    b = _funnel_batch()
    no_stats, none = b.draw_summary(60, stats=False)
    b.close()
    b = _funnel_batch()
    plain, st_plain = b.draw_summary(60, False, True, 32, None, False)
    b.close()
    return with_diag, st_diag, no_stats, none, plain, st_plain


def _same_summary(a, b):
    for f in dataclasses.fields(N.Summary):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and (u64(x) == u64(y)).all(), f.name
        else:
            assert x == y, f.name


def test_draw_summary_diagnostics_equal_the_restatement_of_the_returned_statistics(engine_runs):
    with_diag, st, *_ = engine_runs
    d = with_diag.sampler
    assert isinstance(d, N.SamplerDiagnostics) and d.phase == "all"
    # (draw_summary hands unwritten rows back zeroed: the funnel run has none, every chain is healthy)
    assert (st["chain_status"] == 0).all()
    want = diag_ref.diagnose(st, diag_ref.ALL, max_events=4096, bfmi_threshold=0.3)
    for i, k in enumerate(DIAG_CHAIN_COUNTS):
        assert (getattr(d, k) == want.chain_counts[:, i]).all(), k
    for i, k in enumerate(DIAG_CHAIN_VALUES):
        assert (u64(getattr(d, k)) == u64(want.chain_values[:, i])).all(), k
    for i, k in enumerate(DIAG_POOLED_COUNTS):
        assert getattr(d, "pooled_" + k) == int(want.pooled_counts[i]), k
    for i, k in enumerate(DIAG_POOLED_VALUES):
        assert u64(np.float64(getattr(d, "pooled_" + k))) == u64(want.pooled_values[i]), k
    assert d.n_events == want.n_events and (d.events == want.events).all() and (d.depth_hist == want.depth_hist).all()
    assert d.pooled_healthy == 128 and d.pooled_rows == 128 * 60 and 0.3 < d.pooled_mean_accept < 1.0 and (d.bfmi > 0).all()


def test_draw_summary_without_host_statistics(engine_runs):
    with_diag, st, no_stats, none, plain, st_plain = engine_runs
    assert none is None and type(no_stats) is N.Summary and no_stats.sampler is None
    _same_summary(no_stats, plain)
    _same_summary(with_diag, plain)
    assert st.tobytes() == st_plain.tobytes()


def test_draw_summary_by_default_attaches_nothing(engine_runs):
    *_, plain, st_plain = engine_runs
    assert type(plain) is N.Summary and plain.sampler is None and "sampler" not in vars(plain)
    assert [f.name for f in dataclasses.fields(plain)] == [f.name for f in dataclasses.fields(N.Summary)] and len(dataclasses.fields(plain)) == 13
    assert st_plain.dtype == N.STATS_DTYPE and st_plain.shape == (60, 128)
