"""The loads of a trajectory's start point on the (16 doubles, 1 wavefront) tiling with gradient-free points (nuts_kernels.hpp `nog_mode`):
the leapfrogs that start at the initial point stream its g_z from the chain's state (leapfrog's GMODE 2: the draw's first leapfrog, and the
first leapfrog of the first doubling that goes the other way), and the draw reads the point's z from the state unless it re-whitens.  The
cases pin both sites, both arms of the pass (dim 1024: the full tile; dim 513: the partly filled tile and descriptor range), both builds of the
kernel (general and sampling) and the re-whitening draws, bit for bit against the oracle: positions and every statistics field."""
import functools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_chains, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

N_CHAINS, NUM_TUNE, N_POST = 3, 12, 30
N_DRAWS = NUM_TUNE + N_POST
DIMS = [513, 1024]
DENS = ["iid", "diag"]


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def make_settings(dim, **kw):
    return N.DiagNutsSettings(num_chains=N_CHAINS, seed=700 + dim % 83, num_tune=NUM_TUNE, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(dens, dim, maxdepth):
    """one oracle run per (density, dim, maxdepth), shared by the cases that compare against it"""
    from oracle import oracle as O
    s, logp = make_settings(dim, maxdepth=maxdepth), make_logp(dens, dim)
    x0 = O.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    pos, st, _, failed = O.run(oracle_settings(O, s), logp.kind, dim, logp.params, O.gpu_cfg(64), N_CHAINS, x0, N_DRAWS, n_threads=N_CHAINS)
    assert failed == 0
    pos.setflags(write=False)
    st.setflags(write=False)
    return x0, pos, st


def engine_run(dens, dim, maxdepth, counts):
    """the run on the engine, one draw_many per entry of `counts` -> positions, statistics, launches of the sampling build per call"""
    x0 = oracle_run(dens, dim, maxdepth)[0]
    b = N.ChainBatch(make_settings(dim, maxdepth=maxdepth), make_logp(dens, dim), N_CHAINS)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (16, 64)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos, st, served = [], [], []
    for k in counts:
        before = sampling_launches(b)
        p, q = b.draw_many(k)
        pos.append(p)
        st.append(q)
        served.append(sampling_launches(b) - before)
    b.close()
    return np.concatenate(pos), np.concatenate(st), served


def both_restart_sites_ran(st):
    """On the oracle's rows: some chain has a draw of depth >= 2 whose selected point lies behind the initial point and one whose selected
    point lies ahead of it — its trajectories of two and more doublings went both ways from the initial point, so the first leapfrog of a
    draw (depth 0) and the first leapfrog of a later doubling towards the other side both started at the initial point."""
    deep = st["depth"] >= 2
    idx = st["index_in_trajectory"]
    return bool((((idx < 0) & deep).any(axis=0) & ((idx > 0) & deep).any(axis=0)).any())


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_both_restart_sites_default_maxdepth(oracle, dens, dim):
    """(a) trajectories of several doublings, both ways: the depth-0 site and the first doubling the other way, general and sampling build"""
    _, pos_o, st_o = oracle_run(dens, dim, 10)
    assert both_restart_sites_ran(st_o[:NUM_TUNE + 1]), "no warm-up draw pair of depth >= 2 on both sides (general kernel)"
    assert both_restart_sites_ran(st_o[NUM_TUNE + 1:]), "no sampling draw pair of depth >= 2 on both sides (sampling build)"
    pos_g, st_g, served = engine_run(dens, dim, 10, [N_DRAWS])
    assert served == [1]
    assert_bit_exact(pos_g, st_g, pos_o, st_o)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_depth_zero_site_alone(oracle, dens, dim):
    """(b) maxdepth 1: every draw is the initial point and one leaf — the depth-0 site on every draw, no other leapfrog"""
    _, pos_o, st_o = oracle_run(dens, dim, 1)
    assert (st_o["depth"] <= 1).all() and (st_o["n_steps"] == 1).all()
    pos_g, st_g, served = engine_run(dens, dim, 1, [N_DRAWS])
    assert served == [1]
    assert_bit_exact(pos_g, st_g, pos_o, st_o)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_rewhitening_draws_on_the_general_kernel(oracle, dens, dim):
    """(c) the warm-up alone, in launches the general kernel serves: after a mass-matrix update the next draw re-whitens — z and g_z of the
    initial point are computed from x and g_x with the new transformation, and the stored z is stale until then"""
    _, pos_o, st_o = oracle_run(dens, dim, 10)
    updates = st_o["transformation_update_id"][:NUM_TUNE]
    assert (updates >= 0).any() and len(np.unique(st_o["transformation_index"][:NUM_TUNE + 1])) > 2, "the warm-up has no mass-matrix update"
    pos_g, st_g, served = engine_run(dens, dim, 10, [5, NUM_TUNE - 5])
    assert served == [0, 0]
    assert_bit_exact(pos_g, st_g, pos_o[:NUM_TUNE], st_o[:NUM_TUNE])


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_set_position_in_the_sampling_phase(oracle, dens, dim):
    """(d) set_position after the warm-up, then more draws: one re-whitening draw of the general kernel from the new point, then the
    sampling build again, its start point read from the state that draw left"""
    s, logp = make_settings(dim), make_logp(dens, dim)
    x0 = oracle_run(dens, dim, 10)[0]
    x1 = oracle.init_positions_uniform(s.seed + 1, 0, N_CHAINS, dim)
    b = N.ChainBatch(s, logp, N_CHAINS)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (16, 64)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_a, st_a = b.draw_many(NUM_TUNE + 6)
    assert sampling_launches(b) == 1
    assert (b.set_position(x1, raise_on_error=False) == 0).all()
    pos_b, st_b = b.draw_many(8)                          # one general draw, seven of the sampling build, in one call
    assert sampling_launches(b) == 2
    pos_c, st_c = b.draw_many(4)
    assert sampling_launches(b) == 3
    b.close()
    pos_o, st_o, _ = oracle_chains(oracle, s, logp, [("set", x0), ("draw", NUM_TUNE + 6), ("set", x1), ("draw", 12)], N_CHAINS)
    assert_bit_exact(np.concatenate([pos_a, pos_b, pos_c]), np.concatenate([st_a, st_b, st_c]), pos_o, st_o)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_launches_of_one_draw(oracle, dens, dim):
    """(e) the run of (a) cut into launches of one draw: every draw's start point comes from the state the launch before it stored"""
    _, pos_o, st_o = oracle_run(dens, dim, 10)
    pos_g, st_g, served = engine_run(dens, dim, 10, [1] * N_DRAWS)
    assert served == [0] * (NUM_TUNE + 1) + [1] * (N_POST - 1)
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
