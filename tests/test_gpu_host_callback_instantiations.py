"""Every kernel instantiation of the host-callback family is run against the oracle at least once, on purpose.

NM_LOGP_HOST_CALLBACK is the only route for a density this library has not compiled, and csrc/kern_host_cb.hip, kern_lr_host_cb.hip and
kern_kin_host_cb.hip instantiate `HostCb`, `LrWrap<HostCb>` and `KinWrap<HostCb>` for all eight tilings of nuts_launch.hpp: 24 draw kernels
plus their init kernels.  test_gpu_host_callback.py runs dims 3 to 6, the (2, 1) tiling of each wrapper; test_gpu_wide_chains.py runs the
separate cluster-mode build.  The code that depends on the tiling is `HostCb::eval` (csrc/nuts_kernels.hpp): the `elem_index<W>(k)` mapping
of register slots to mailbox words on the store of x and the load of the gradient, the `d < dim` guards of a ragged last tile, the block-wide
synchronisation before the request is published, thread 0 alone ringing and polling with the failure flag spread through a block sum, and the
status read per wavefront.  A miscompile is a per-instantiation event, so the guard is per instantiation here too:

    {DiagNutsSettings, LowRankNutsSettings frozen / adapting, ExactNormal, Microcanonical, MCLMC, LowRank MCLMC}
        x  the eight tilings (doubles per lane, wavefronts per chain)  x  both ends of the tiling's range of dims

This family has NO known answers as data (nuts_rs_amd/selftest_instantiations.json holds the built-in densities only): a Python callback has
none, `selftest.first_use` checks nothing for these engines, and oracle parity — this file — is the family's only guard.

The density is one plain-numpy function on both sides.  It ties every coordinate to its neighbours (across lane, wavefront and tile borders)
and weights coordinate i by its index, so it is not invariant under a permutation of coordinates: a wrong slot-to-word mapping changes the
draws.  The second part of the file runs the reference's error taxonomy (a recoverable error is a divergence without an energy error, an
unrecoverable one stops the chain: src/dynamics/transformed_hamiltonian.rs:562-578, src/nuts.rs:231) on the multi-wavefront tilings, keyed
on the LAST coordinate, which the last lanes of the last wavefront own.

No case is skipped: seeds, walls and fatal regions are chosen with the oracle alone (tools/small_chain_dry_run.py --only hostcb), and the
tests assert what that pass reports.  The draw every kernel restates: reference src/chain.rs:150-243.

Measured on an MI355X: the 96 cases take 30 s together; the slowest is lr_adapt-4x1-dim256 at 3.3 s, every non-adapting case is below 2 s.
The engine's share of a case is about the oracle's own (dim 4096, ~870 callbacks: 0.34 s against 0.31 s; dim 2, ~1200 callbacks: 0.02 s, i.e.
under 20 us per evaluation with the mailbox round trip in it): the time is the Python callback's on both sides, not the round trip's.  Each case
prints its two times (`pytest -s`)."""
import time

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import selftest_cases as SC
from helpers import assert_bit_exact, estimator_pair, oracle_settings
from test_gpu_every_instantiation import generic_transform
from test_gpu_host_callback import compare, run_both, run_oracle_chains

pytestmark = pytest.mark.gpu

N_CHAINS = 3
NUM_TUNE, N_DRAWS, MAXDEPTH = 12, 20, 4          # the callback is Python on both sides: short runs (a dim-4093 case: 0.6 s in the oracle)
LR_MCLMC_TUNE = 50                               # LowRank MCLMC: half of `SC.make_run`'s warm-up (measured: see make_run)
# a case whose default seed gives a rejected initial point, a failed oracle chain or trees below depth 3 (tools/small_chain_dry_run.py
# --only hostcb) gets another one here, by id
SEEDS = {}
# (family, tiling) combinations `plan_engine` refuses for NM_LOGP_HOST_CALLBACK, with the plan's own message: "fam-DPLxW" -> message.
# Such a case asserts NutsAmdError instead of running.  (None at this revision: every family has its host-callback kernels on every tiling.)
REFUSED = {}


def coupled(chain, x):
    """a random-walk prior (every coordinate tied to its neighbour) plus an index-weighted normal and a weak quartic well: `_coupled` of
    test_gpu_wide_chains.py with weights that depend on the coordinate's index.  Deterministic numpy arithmetic on a fresh copy, so that the
    engine's and the oracle's calls compute on arrays of the same alignment and agree bit for bit."""
    x = np.array(x); w = 1.0 + (np.arange(len(x)) % 7) / 8.0; d = np.diff(x)
    lp = -2.0 * float(np.dot(d, d)) - 0.125 * float(np.dot(w * x, x)) - 0.01 * float(np.sum(x ** 4))
    g = -0.25 * w * x - 0.04 * x ** 3
    g[:-1] += 4.0 * d; g[1:] -= 4.0 * d
    return lp, g


def hostcb_cases():
    """The tilings, families and dim ends of the package's own list (its iid rows), so that neither can drift."""
    return [dict(c, dens="hostcb") for c in SC.cases() if c["dens"] == "iid"]


def make_run(c):
    """-> (settings, draws, adapting).  The adapting families run at dim <= 256, where a callback costs microseconds: `SC.make_run`'s own
    settings (num_tune 100, 110 draws, mass_matrix_update_freq 5; LowRank MCLMC: 50 + 5 draws).  Every other family: 12 warm-up draws + 8,
    trees to depth 4."""
    fam = c["fam"]
    r = SC.make_run(N, dict(c, dens="iid"))
    seed = SEEDS.get(SC.case_id(c), r["settings"].seed)
    if fam in ("lr_adapt", "lr_mclmc"):
        s = r["settings"]
        s.seed = seed
        if fam == "lr_mclmc":      # its estimator runs after every warm-up draw of every chain, on both sides: at 100 warm-up draws 8 s a case, all LAPACK
            s.num_tune = LR_MCLMC_TUNE
            return s, LR_MCLMC_TUNE + 5, True
        return s, r["draws"], True
    kw = dict(num_chains=N_CHAINS, seed=seed, num_tune=NUM_TUNE)
    if fam == "mclmc":
        s = N.DiagMclmcSettings(step_size=0.05, momentum_decoherence_length=1.0, **kw)
    elif fam == "lr_frozen":
        s = N.LowRankNutsSettings(freeze_transform=True, maxdepth=MAXDEPTH, **kw)
    else:
        s = N.DiagNutsSettings(maxdepth=MAXDEPTH, trajectory_kind={"nuts": 0, "exact": 1, "micro": 2}[fam], **kw)
    return s, N_DRAWS, False


def make_transform(c, s):
    """lr_frozen: full-mantissa doubles, as in test_instantiation_bit_exact_generic_inputs"""
    return generic_transform(c["dim"], np.random.default_rng(s.seed + 7)) if c["fam"] == "lr_frozen" else None


def oracle_side(O, c, s, draws, x0, tpc, order=0, estimator=None):
    """One oracle chain per engine chain on `coupled`, in the order of `nmo_run_ex` (oracle/nuts_oracle.cpp): the estimator, set_position,
    the transformation given from outside, the draws.  -> positions [draws][chains][dim], statistics, chains that failed, seconds."""
    dim, n = c["dim"], len(x0)

    def tramp(ctx, d, px, pg, plogp):
        lp, g = coupled(0, np.ctypeslib.as_array(px, shape=(d,)).copy())
        np.ctypeslib.as_array(pg, shape=(d,))[:] = g
        plogp[0] = lp
        return 0
    cb = O.HOST_LOGP_FN(tramp)
    so = oracle_settings(O, s)
    transform = make_transform(c, s)
    pos = np.full((draws, n, dim), np.nan)
    st = np.zeros((draws, n), dtype=O.STATS_DTYPE)
    failed = []
    t0 = time.perf_counter()
    for k in range(n):
        ch = O.Chain(so, 0, dim, np.zeros(1), O.gpu_cfg(tpc, lr_seq_dots=order if transform is not None else 0), chain_id=k, callback=cb)
        if estimator is not None:
            ch.set_estimator(estimator)
        if ch.set_position(x0[k]) != 0:
            failed.append(k)
            continue
        if transform is not None:
            assert ch.set_transform(*transform) == 1
        for t in range(draws):
            pos[t, k], st[t, k], rc = ch.draw()
            if rc != 0:
                failed.append(k)
                break
    return pos, st, failed, time.perf_counter() - t0


def tiling_id(c):
    return f"{c['fam']}-{c['dpl']}x{c['w']}"


@pytest.mark.parametrize("case", [pytest.param(c, id=SC.case_id(c)) for c in hostcb_cases()])
def test_host_callback_instantiation_bit_exact(oracle, case):
    O = oracle
    dim, dpl, w = case["dim"], case["dpl"], case["w"]
    s, draws, adapting = make_run(case)
    calls = []                                   # (list.append is atomic: the engine calls from two service threads)

    def counted(chain, x):
        calls.append(chain)
        return coupled(chain, x)
    kw = dict(dims_per_lane=dpl, waves_per_chain=w, lane_groups=1, lane_chains=1, chain_tiles=1)      # the one-chain-per-block kernels, nothing else
    if tiling_id(case) in REFUSED:
        with pytest.raises(N.NutsAmdError):
            N.ChainBatch(s, N.LogpSpec.host_callback(dim, counted, threads=2), N_CHAINS, **kw)
        return
    t0 = time.perf_counter()
    b = N.ChainBatch(s, N.LogpSpec.host_callback(dim, counted, threads=2), N_CHAINS, **kw)
    try:
        assert (b.dims_per_lane(), b.threads_per_chain() // 64) == (dpl, w) and b.blocks_per_chain() == 1
        x0 = O.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
        status = b.set_position(x0, raise_on_error=False)
        assert (status == 0).all(), "the engine rejected an initial point: pick another seed for this case (SEEDS)"
        transform = make_transform(case, s)
        cb_o = None
        if adapting:
            cb_o, cb_e, rec = estimator_pair(O)
            b.set_lowrank_estimator(cb_e, n_threads=1)
        elif transform is not None:
            b.set_transform(*transform)
        cut = draws // 2
        pa, sa = b.draw_many(cut, raise_on_error=False)
        pb, sb = b.draw_many(draws - cut, raise_on_error=False)           # the chains' state survives the end of a launch
        pos, st = np.concatenate([pa, pb]), np.concatenate([sa, sb])
        tpc, order = b.threads_per_chain(), b.reduce_order()
        steps, host_calls = b.counters()["total_leapfrogs"], b.host_logp_calls()
    finally:
        b.close()
    t_engine = time.perf_counter() - t0
    n_engine, n_estimates = len(calls), len(rec) if adapting else 0
    pos_o, st_o, failed, t_oracle = oracle_side(O, case, s, draws, x0, tpc, order, cb_o)
    print(f"{SC.case_id(case)}: engine {t_engine:.2f} s ({n_engine} callbacks, {steps} leapfrogs), oracle {t_oracle:.2f} s")
    assert not failed, f"oracle chains {failed} failed: pick another seed for this case (SEEDS)"
    assert_bit_exact(pos, st, pos_o, st_o)
    if case["fam"] in ("mclmc", "lr_mclmc"):
        for f in ("energy_change", "average_step_size"):
            assert ((st[f] == st_o[f]) | (np.isnan(st[f]) & np.isnan(st_o[f]))).all(), f
    assert host_calls == n_engine                                  # one call per gradient per chain, not one per wavefront
    assert set(calls) == set(range(N_CHAINS)) and host_calls >= steps + N_CHAINS
    assert steps == int(st_o["n_steps"].sum())
    assert st["depth"].max() >= 3 and (st["chain_status"] == 0).all()
    if adapting:       # the estimator ran, as often on one side as on the other
        assert n_estimates >= N_CHAINS and len(rec) == 2 * n_estimates


# ---- the error taxonomy on the multi-wavefront tilings -----------------------------------------------------------------------------------------
# (16, 1), (8, 2), (4, 4) share the cap 1024; all four run a ragged top dim.  The wall and the fatal region are keyed on x[dim - 1].
TAXONOMY_TILINGS = [(16, 1), (8, 2), (4, 4), (16, 4)]
TAX_CHAINS, TAX_TUNE, TAX_DRAWS, TAX_MAXDEPTH = 4, 16, 32, 5
WALL = 1.25                 # recoverable beyond it: a unit normal's last coordinate meets it within a few draws
FATAL = -2.0                # unrecoverable below it
# per case id: the seed (chosen by tools/small_chain_dry_run.py --only hostcb: the wall is met, and in the fatal cases some chains stop and some go on)
TAX_SEEDS = {}


def taxonomy_cases():
    return [dict(kind=kind, dpl=d, w=w, dim=d * 64 * w - 3) for kind in ("recoverable", "fatal") for (d, w) in TAXONOMY_TILINGS]


def taxonomy_id(c):
    return f"{c['kind']}-{c['dpl']}x{c['w']}-dim{c['dim']}"


def taxonomy_seed(c):
    return TAX_SEEDS.get(taxonomy_id(c), 40 + 7 * c["dpl"] + c["w"])


def taxonomy_density(c):
    """`walled` / `fatal_later` of test_gpu_host_callback.py on a unit normal, keyed on the last coordinate.  The fatal cases keep the wall:
    every case has divergences without an energy error."""
    last, fatal = c["dim"] - 1, c["kind"] == "fatal"

    def density(chain, x):
        if x[last] > WALL:
            raise N.RecoverableLogpError("outside the support")
        if fatal and x[last] < FATAL:
            raise ValueError("not recoverable")
        return -0.5 * float(np.dot(x, x)), -x
    return density


def taxonomy_oracle(O, c):
    """The oracle's side alone (the dry run): what `run_both` computes for the case, and its settings."""
    s = N.DiagNutsSettings(num_chains=TAX_CHAINS, seed=taxonomy_seed(c), num_tune=TAX_TUNE, store_divergences=True, maxdepth=TAX_MAXDEPTH)
    x0 = O.init_positions_uniform(s.seed, 0, TAX_CHAINS, c["dim"])
    return run_oracle_chains(O, taxonomy_density(c), s, c["dim"], TAX_CHAINS, TAX_DRAWS, x0, 64 * c["w"])


def taxonomy_findings(c, res):
    """What the oracle's chains must show for the case to test anything: -> a list of complaints (empty: fine)."""
    out = []
    if any(rc != 0 for rc, _ in res):
        out.append("an initial point is rejected")
    nan_div = sum(1 for rc, rows in res for (_, q, rc2) in rows if rc2 == 0 and q["diverging"] and np.isnan(q["divergence_energy_error"]))
    if nan_div == 0:
        out.append("the wall is never met (no divergent draw without an energy error)")
    stopped = [k for k, (rc, rows) in enumerate(res) if rows and rows[-1][2] != 0]
    if c["kind"] == "fatal":
        if not stopped:
            out.append("no chain meets the fatal region")
        if len(stopped) == len(res):
            out.append("every chain stops: none is left to go on")
        if any(len(res[k][1]) == TAX_DRAWS for k in stopped):
            out.append("a chain stops in the last draw: no later draw to look at")
    elif stopped:
        out.append("a chain stops in a recoverable case")
    return out


@pytest.mark.parametrize("case", [pytest.param(c, id=taxonomy_id(c)) for c in taxonomy_cases()])
def test_error_taxonomy_on_multi_wavefront_tilings(oracle, case):
    dim, fatal = case["dim"], case["kind"] == "fatal"
    fn = taxonomy_density(case)
    status, pos, st, res, _ = run_both(oracle, fn, fn, dim, TAX_CHAINS, TAX_TUNE, TAX_DRAWS, seed=taxonomy_seed(case),
                                       dims_per_lane=case["dpl"], waves_per_chain=case["w"], maxdepth=TAX_MAXDEPTH)
    assert taxonomy_findings(case, res) == [], "pick another seed for this case (TAX_SEEDS; tools/small_chain_dry_run.py --only hostcb)"
    compare(status, pos, st, res, allow_stop=fatal)
    stopped = {k: len(rows) - 1 for k, (rc, rows) in enumerate(res) if rows[-1][2] != 0}       # chain -> the draw in which the oracle stops it
    cs = st["chain_status"]
    live = np.ones(cs.shape, dtype=bool)                                    # the draws a chain completed
    for k in range(TAX_CHAINS):
        if k in stopped:
            t = stopped[k]
            live[t:, k] = False
            assert res[k][1][t][2] == 2 and cs[t, k] == 2                   # NM_CHAIN_LOGP_FATAL, in the oracle's draw
            assert (cs[:t, k] == 0).all() and (st["n_steps"][:t, k] > 0).all()
            assert (st["n_steps"][t + 1:, k] == 0).all()                    # ... and nothing runs afterwards
        else:
            assert (cs[:, k] == 0).all() and (st["n_steps"][:, k] > 0).all() and np.isfinite(pos[:, k]).all()      # the other chains go on
    assert fatal == bool(stopped)
    div = (st["diverging"] != 0) & live
    assert (div & np.isnan(st["divergence_energy_error"])).sum() >= 1       # a recoverable error: a divergence that carries no energy error
    assert (pos[..., dim - 1][live] <= WALL).all()
    if fatal:
        assert (pos[..., dim - 1][live] >= FATAL).all()
