"""The chain's scalar step-size protocol (DualAverage / Adam new + advance, update_stepsize with its jitter draw, the next-window rule, the
collector's last_* values, the row's step_size_bar: nuts_rs_amd/csrc/nuts_adapt.hpp for the lane and lockstep kernels, the wave and group
kernels' own statements of the same lines) on every kernel family that runs it, with every step-size method, with and without jitter,
bit for bit against the oracle.  tests/test_gpu_lane_chains.py::test_lane_kernel_sweep randomises
the same for the one-chain-per-lane family; here are the others, on the smallest shapes that reach them:

  wave_small   one wavefront per chain, tiling (2, 1): `adapt` of the small units
  wave_large   tiling (16, 1): `adapt` of the large units and, after the warm-up, the sampling-phase build
  wave_lr      LowRankNutsSettings: `adapt_lr` / `adapt_tail` with the pause for the host's estimator
  group        8 lanes per chain: `g_adapt`
  lockstep     the matrix-core lockstep kernel with a frozen shared transformation: `adapt_frozen`

A warm-up of 60 draws (early window 18 draws with switches every 5, then windows of 10 growing by 1.5 — 15, then round(22.5) = 23 —, the
final step-size window from draw 51) and 20 draws after it, cut into launches at 60 and 61, crosses every arm of the schedule: early,
window switches, the round-half-away rule, is_late, the final step-size window, draw == num_tune - 1 and draw >= num_tune."""
import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import (assert_bit_exact, correlated_precision, estimator_pair, oracle_settings, run_engine, run_oracle, run_fixed,
                     sampling_launches)

pytestmark = pytest.mark.gpu

TUNE, DRAWS, SPLITS = 60, 80, (60, 61)
METHODS = {"dual_average": N.STEP_DUAL_AVERAGE, "adam": N.STEP_ADAM, "fixed": N.STEP_FIXED}


def protocol_settings(method, jitter, n_chains, seed, low_rank=False, **kw):
    st = N.StepSizeSettings(method=METHODS[method], jitter=jitter, fixed_step_size=0.05)
    ao = N.EuclideanAdaptOptions(step_size_settings=st, early_window=0.3, step_size_window=0.15, mass_matrix_switch_freq=10,
                                 early_mass_matrix_switch_freq=5, mass_matrix_window_growth=1.5)
    make = N.LowRankNutsSettings if low_rank else N.DiagNutsSettings
    return make(num_chains=n_chains, seed=seed, num_tune=TUNE, num_draws=DRAWS - TUNE, adapt_options=ao, **kw)


def diag_normal(dim):
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def check_inputs(st_o, failed, frozen=False):
    """Conditions on the chosen inputs (not tolerances): the run crosses what it is meant to cross."""
    assert failed == 0
    assert st_o["tuning"][:TUNE].all() and not st_o["tuning"][TUNE:].any()                  # `tuning` flips at draw 60
    if not frozen:                              # the transformation changed at least twice during the warm-up (its first event is the initial one)
        assert ((st_o["transformation_update_id"][:TUNE] >= 0).sum(axis=0) >= 3).all()


jitters = pytest.mark.parametrize("jitter", [0.1, None], ids=["jitter", "no_jitter"])
methods = pytest.mark.parametrize("method", list(METHODS))


@methods
@jitters
@pytest.mark.parametrize("family", ["wave_small", "wave_large", "group"])
def test_diag_families_bit_exact(oracle, family, method, jitter):
    # (the seeds: with a fixed step size a chain whose start has a coordinate very close to 0 — an enormous first scale from the gradient —
    #  diverges on every draw and never moves its transformation; check_inputs rejects such a start)
    dim, n, seed, kw = {"wave_small": (70, 3, 44, {}), "wave_large": (600, 2, 44, {}),
                        "group": (9, 70, 41, dict(lane_chains=1, lane_groups=2))}[family]
    s = protocol_settings(method, jitter, n, seed=seed)
    logp = diag_normal(dim)
    x0 = oracle.init_positions_uniform(s.seed, 0, n, dim)
    pos_o, st_o, steps, failed = run_oracle(oracle, s, logp, n, x0, DRAWS)
    check_inputs(st_o, failed)
    if family == "wave_large":                   # (run_engine closes the engine: the sampling build's counter is read before)
        b = N.ChainBatch(s, logp, n)
        assert (b.set_position(x0) == 0).all() and (b.dims_per_lane(), b.threads_per_chain()) == (16, 64)
        parts = [b.draw_many(k) for k in (60, 1, 19)]
        assert sampling_launches(b) > 0
        b.close()
        pos_g, st_g = np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])
    else:
        pos_g, st_g, ex = run_engine(s, logp, n, x0, DRAWS, splits=SPLITS, **kw)
        assert (ex["status"] == 0).all() and ex["lane_launches"] == 0
        if family == "group":
            assert ex["group_launches"] > 0
        else:
            assert ex["group_launches"] == 0 and (ex["dims_per_lane"], ex["threads_per_chain"]) == (2, 64)
        assert ex["counters"]["total_leapfrogs"] == steps
    assert_bit_exact(pos_g, st_g, pos_o, st_o)


@methods
@jitters
def test_lowrank_adapt_bit_exact(oracle, method, jitter):
    """`adapt_lr`: the schedule and the step-size part on the device, the estimator on the host (the oracle's, on both sides)."""
    n, dim = 3, 10
    s = protocol_settings(method, jitter, n, seed=43, low_rank=True)
    logp = diag_normal(dim)
    cb_o, cb_e, rec = estimator_pair(oracle)
    x0 = oracle.init_positions_uniform(s.seed, 0, n, dim)
    b = N.ChainBatch(s, logp, n)
    assert (b.set_position(x0) == 0).all()
    b.set_lowrank_estimator(cb_e, n_threads=1)
    parts = [b.draw_many(k) for k in (60, 1, 19)]
    pos_g, st_g = np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])
    tpc = b.threads_per_chain()
    n_eng = len(rec)
    b.close()
    pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, s), logp.kind, logp.dim, logp.params, oracle.gpu_cfg(tpc), n, x0, DRAWS, estimator=cb_o)
    check_inputs(st_o, failed)
    assert len(rec) == 2 * n_eng and n_eng >= 2 * n             # both sides asked the estimator equally often
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    assert (st_g["num_eigenvalues"] == st_o["num_eigenvalues"]).all()


@methods
@jitters
def test_lockstep_frozen_bit_exact(oracle, method, jitter):
    """`adapt_frozen` of the lockstep kernel: a shared, frozen low-rank transformation, 21 chains (a ragged second tile)."""
    dim, rank, n = 64, 16, 21
    rng = np.random.default_rng(dim + rank)
    prec, sigma = correlated_precision(rng, dim, 4)
    w, u = np.linalg.eigh(sigma)
    keep = np.argsort(np.abs(np.log(w)))[::-1][:rank]
    tr = (np.exp(rng.normal(0, 0.2, dim)), rng.normal(0, 0.5, dim), w[keep], np.ascontiguousarray(u[:, keep].T), rng.normal(0, 0.1, dim))
    s = protocol_settings(method, jitter, n, seed=47, low_rank=True, freeze_transform=True)
    pos_g, st_g, pos_o, st_o = run_fixed(oracle, N.LogpSpec.mvn_precision(prec), s, n, tr, DRAWS, expect_tiles=True, expect_order=2, splits=SPLITS,
                                         chain_tiles=0)           # (run_fixed asserts that no chain failed its init on either side)
    check_inputs(st_o, 0, frozen=True)
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
