"""The sampling-phase build of the wave-per-chain draw kernel (K_DRAW_SAMPLING: nuts_kernels.hpp `SAMPLING`, nuts_engine.hip
`sampling_from`): the draws with an index > num_tune run on a kernel without the warm-up's code.  Whatever way a run is cut into
launches, positions and every statistics field are the oracle's bits, and the debug counter shows which kernel served which draws."""
import functools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, assert_vectors_bit_exact, oracle_chains, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

N_CHAINS, NUM_TUNE, N_POST = 3, 12, 10
N_DRAWS = NUM_TUNE + N_POST                      # draw indices 0 .. 21: 12 .. 21 come after the warm-up, 13 .. 21 may take the sampling build
# both ends of the (16 doubles, 1 wavefront) tiling, both ends of the (8, 1) tiling
DIMS = [(513, 16), (1024, 16), (257, 8), (512, 8)]
SPLITS = {"one_launch": [N_DRAWS], "launches_of_1": [1] * N_DRAWS, "launches_of_5": [5, 5, 5, 5, 2]}


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def make_settings(dim, **kw):
    kw.setdefault("num_tune", NUM_TUNE)
    return N.DiagNutsSettings(num_chains=N_CHAINS, seed=300 + dim % 89, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(dens, dim):
    """one oracle run per (density, dim), shared by the three ways of cutting it into launches"""
    from oracle import oracle as O
    s, logp = make_settings(dim), make_logp(dens, dim)
    x0 = O.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    pos, st, _, failed = O.run(oracle_settings(O, s), logp.kind, dim, logp.params, O.gpu_cfg(64), N_CHAINS, x0, N_DRAWS, n_threads=N_CHAINS)
    assert failed == 0
    pos.setflags(write=False)
    st.setflags(write=False)
    return x0, pos, st


def draw_in_launches(b, counts, num_tune):
    """draw_many per entry of `counts`; checks after every call which kernel served it: none of the sampling build while the call has no
    draw past index num_tune (the draw AT num_tune is the general kernel's), exactly one as soon as it has"""
    pos, st, lo = [], [], 0
    for k in counts:
        before = sampling_launches(b)
        p, q = b.draw_many(k)
        pos.append(p)
        st.append(q)
        last = lo + k - 1
        assert sampling_launches(b) - before == (1 if last > num_tune else 0), (lo, k)
        lo += k
    return np.concatenate(pos), np.concatenate(st)


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("dim,dpl", DIMS, ids=[f"dim{d}" for d, _ in DIMS])
@pytest.mark.parametrize("dens", ["iid", "diag"])
def test_boundary_in_every_position_bit_exact(oracle, dens, dim, dpl, split):
    x0, pos_o, st_o = oracle_run(dens, dim)
    b = N.ChainBatch(make_settings(dim), make_logp(dens, dim), N_CHAINS)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (dpl, 64)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_g, st_g = draw_in_launches(b, SPLITS[split], NUM_TUNE)
    total = sampling_launches(b)
    b.close()
    assert total > 0
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    # the boundary is where the test thinks it is: the warm-up's rows, the one general row after it, the sampling rows
    assert (st_g["tuning"][:NUM_TUNE] == 1).all() and (st_g["tuning"][NUM_TUNE:] == 0).all()
    assert (st_g["transformation_update_id"][NUM_TUNE + 1:] == -1).all()


def test_set_position_in_the_sampling_phase_goes_back_to_the_general_kernel(oracle):
    """set_position gives the chain a new mass matrix (from the gradient) and the step size of a new search: the next draw re-whitens,
    reports the transformation and replaces the step size — the general kernel's work.  After that draw the state is frozen again."""
    dim = 600
    s, logp = make_settings(dim), make_logp("diag", dim)
    x0 = oracle.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    x1 = oracle.init_positions_uniform(s.seed + 1, 0, N_CHAINS, dim)
    b = N.ChainBatch(s, logp, N_CHAINS)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_a, st_a = draw_in_launches(b, [NUM_TUNE + 4], NUM_TUNE)
    assert sampling_launches(b) == 1
    assert (b.set_position(x1, raise_on_error=False) == 0).all()
    pos_b, st_b = b.draw_many(1)
    assert sampling_launches(b) == 1                       # the first draw after set_position: general kernel
    pos_c, st_c = b.draw_many(4)
    assert sampling_launches(b) == 2
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_d, st_d = b.draw_many(3)                           # ... also inside a launch: one general draw, two of the sampling build
    assert sampling_launches(b) == 3
    b.close()
    pos_o, st_o, _ = oracle_chains(oracle, s, logp, [("set", x0), ("draw", NUM_TUNE + 4), ("set", x1), ("draw", 5), ("set", x0), ("draw", 3)], N_CHAINS)
    pos_g, st_g = np.concatenate([pos_a, pos_b, pos_c, pos_d]), np.concatenate([st_a, st_b, st_c, st_d])
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    assert (st_b["transformation_update_id"] >= 0).all()   # the draw after set_position did have the general kernel's work to do


def test_shortest_warmup_and_frozen_transform(oracle):
    """num_tune = 1, the shortest warm-up there is (num_tune = 0 fails the reference's own assertion early_end < num_tune,
    adapt_strategy.rs:83, and nm_engine_create refuses it: no kernel ever runs): draw 0 adapts, draw 1 = num_tune ends the tuning on the
    general kernel, the sampling build serves the rest.  freeze_transform: the estimators rest during the warm-up, the step size adapts;
    the sampling build takes over after draw num_tune as in any other run."""
    dim = 700
    logp = make_logp("diag", dim)
    with pytest.raises(N.NutsAmdError):
        N.ChainBatch(make_settings(dim, num_tune=0), logp, N_CHAINS)
    for kw, counts in ((dict(num_tune=1), [1, 1, 4]), (dict(num_tune=1), [2, 4]), (dict(num_tune=1), [6]), (dict(freeze_transform=True), [N_DRAWS])):
        s = make_settings(dim, **kw)
        x0 = oracle.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
        b = N.ChainBatch(s, logp, N_CHAINS)
        assert (b.set_position(x0, raise_on_error=False) == 0).all()
        pos_g, st_g = draw_in_launches(b, counts, s.num_tune)
        assert sampling_launches(b) == 1
        b.close()
        pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, s), logp.kind, dim, logp.params, oracle.gpu_cfg(64), N_CHAINS, x0, sum(counts), n_threads=N_CHAINS)
        assert failed == 0
        assert_bit_exact(pos_g, st_g, pos_o, st_o)


# chosen on the oracle alone (a scan over seeds and step sizes on the CPU): of the nine draws the sampling build serves (indices 13 .. 21)
# chain 0 has no divergent one, chain 1 has five, chain 2 nine
DIV_DIM, DIV_SEED, DIV_STEP = 600, 3, 0.13


def test_divergences_on_the_sampling_build(oracle):
    """A fixed step size at which the oracle itself reports divergent and non-divergent draws after the warm-up, with the divergence
    vectors requested (the sampling build then stores x / g_x after every draw, as the general kernel does)."""
    dim = DIV_DIM
    s = N.DiagNutsSettings(num_chains=N_CHAINS, seed=DIV_SEED, num_tune=NUM_TUNE, store_divergences=True)
    s.adapt_options.step_size_settings.method = N.STEP_FIXED
    s.adapt_options.step_size_settings.fixed_step_size = DIV_STEP
    logp = make_logp("diag", dim)
    x0 = oracle.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    vec_o = {}
    pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, s), logp.kind, dim, logp.params, oracle.gpu_cfg(64), N_CHAINS, x0, N_DRAWS, n_threads=N_CHAINS,
                                        vectors=vec_o)
    assert failed == 0
    div_o = st_o["diverging"][NUM_TUNE + 1:] != 0          # the rows of the sampling build
    assert div_o.any() and not div_o.all()
    b = N.ChainBatch(s, logp, N_CHAINS)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_g, st_g, vec_g = b.expanded_draw_many(N_DRAWS)
    assert sampling_launches(b) == 1
    b.close()
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    assert_vectors_bit_exact(vec_g, vec_o)
    assert (np.isnan(vec_g["divergence_start"]).all(axis=2) == (st_g["diverging"] == 0)).all()
