"""pooled_lowrank_warmup end to end: 512 chains on a correlated normal of dim 32 share ONE low-rank transformation estimated
from the pooled windows' scatter matrices (nm_pooled_scatter + lowrank_from_moments), which makes them eligible for the matrix-core draw
kernels.  An identically seeded batch warmed with the existing DIAGONAL pooled_warmup is the yardstick for the trajectory lengths."""
import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import pooled

pytestmark = pytest.mark.gpu

DIM, CHAINS, TUNE, DRAWS, SEED, CUTOFF = 32, 512, 300, 100, 29, 2.0


def correlated_precision(rng, dim, rank, scale=50.0):
    """the target of tests/test_gpu_lowrank.py, restated: unit covariance plus `rank` directions of variance 6 .. 51, rescaled per element"""
    u = np.linalg.qr(rng.normal(size=(dim, rank)))[0]
    sigma = np.eye(dim) + u @ np.diag(rng.uniform(5.0, scale, rank)) @ u.T
    sc = np.exp(rng.normal(0, 0.5, dim))
    sigma = np.diag(sc) @ sigma @ np.diag(sc)
    prec = np.linalg.inv(sigma)
    return (prec + prec.T) / 2, sigma


def warmed(prec, low_rank):
    s = N.LowRankNutsSettings(num_chains=CHAINS, seed=SEED, num_tune=TUNE, freeze_transform=True, eigval_cutoff=CUTOFF)
    b = N.ChainBatch(s, N.LogpSpec.mvn_precision(prec), CHAINS, chain_tiles=2)
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    ups = pooled.pooled_lowrank_warmup(b, TUNE) if low_rank else pooled.pooled_warmup(b, TUNE)
    launches = (b.tile_launches(), b.lockstep_launches())
    pos, st = b.draw_many(DRAWS)
    launches_after = (b.tile_launches(), b.lockstep_launches())
    b.close()
    return ups, pos, st, launches, launches_after


@pytest.fixture(scope="module")
def runs():
    prec, sigma = correlated_precision(np.random.default_rng(SEED), DIM, 4)
    return sigma, warmed(prec, True), warmed(prec, False)


def test_pooled_lowrank_warmup_reaches_the_matrix_core_kernels_and_whitens_the_target(runs):
    sigma, (ups, pos, st, launches, launches_after), (ups_d, pos_d, st_d, launches_d, _) = runs
    assert (st["chain_status"] == 0).all() and (st_d["chain_status"] == 0).all()
    assert len(ups) == len(pooled.window_schedule(TUNE)) == len(ups_d)
    # (a) the matrix-core kernels served the warm-up and the draws after it; the diagonal transformation never reaches them
    assert sum(launches) > 0 and sum(launches_after) > sum(launches)
    assert sum(launches_d) == 0
    at, stds, mean, vals, vecs, mu = ups[-1]
    assert at == sum(pooled.window_schedule(TUNE)) and len(vals) % 8 == 0 and 8 <= len(vals) <= DIM and vecs.shape == (len(vals), DIM)
    # (b) the target whitened by the final transformation: z = F^-1 (x - mean), F = diag(stds) (I + U (lambda^1/2 - 1) U').  For a normal
    # target g is linear in x, so C_g = P C_x P for ANY sample and the estimate is exact up to the eigenvalues the cutoff leaves alone,
    # whose spread is at most cutoff^2; 5 % for gamma and the rounding of eigh at the target's conditioning.
    f_inv = (np.eye(DIM) + (vecs.T * (vals**-0.5 - 1.0)) @ vecs) / stds
    ev = np.linalg.eigvalsh(f_inv @ sigma @ f_inv.T)
    d = np.sqrt(np.diag(sigma))
    print("condition number: whitened", ev.max() / ev.min(), "diagonal scaling", np.linalg.cond(sigma / np.outer(d, d)))
    assert ev.max() / ev.min() <= CUTOFF**2 * 1.05


def test_pooled_lowrank_warmup_shortens_the_trajectories_and_samples_the_target(runs):
    sigma, (ups, pos, st, _, _), (ups_d, pos_d, st_d, _, _) = runs
    # (c) strictly fewer leapfrogs per draw than the diagonal pooled transformation leaves
    steps, steps_d = st["n_steps"].mean(), st_d["n_steps"].mean()
    print("leapfrogs per draw: pooled low-rank", steps, "pooled diagonal", steps_d)
    assert steps < steps_d
    # (d) the pooled mean of every element within 6 standard errors of the target's (0)
    s = N.summarize_draws(pos)
    err = np.abs(s.mean - 0.0) / (s.sd / np.sqrt(s.ess))
    print("largest |mean| in standard errors", err.max(), "smallest ess", s.ess.min())
    assert (err <= 6.0).all()


def test_a_batch_with_a_smaller_lowrank_max_rank_is_served():
    """the estimate is cut to the batch's lowrank_max_rank (nm_engine_set_transform refuses more): 8 of the pairs at dim 32"""
    prec, _ = correlated_precision(np.random.default_rng(SEED), DIM, 12)
    s = N.LowRankNutsSettings(num_chains=64, seed=SEED, num_tune=60, freeze_transform=True, eigval_cutoff=CUTOFF)
    b = N.ChainBatch(s, N.LogpSpec.mvn_precision(prec), 64, chain_tiles=2, lowrank_max_rank=8)
    assert b.lowrank_max_rank() == 8
    assert (b.set_position(b.init_positions_uniform()) == 0).all()
    ups = pooled.pooled_lowrank_warmup(b, 60, windows=[10, 10, 20])
    pos, st = b.draw_many(5)
    b.close()
    assert len(ups) == 3 and all(len(u[3]) <= 8 for u in ups) and len(ups[-1][3]) == 8
    assert (st["chain_status"] == 0).all()
