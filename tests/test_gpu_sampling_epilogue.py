"""Round 8 on the sampling-phase build (nuts_kernels.hpp `SAMPLING`): the merge into the main tree with one exp (dev_math.hpp
merge_math_main).  Engine against oracle, bit for bit on positions and every statistics field, iid and diagonal normal, on both tilings
that have a sampling build: dim 480 (8 doubles per lane), 600, 1000 (a partly filled tile) and 1024 (16 per lane).  The dims are the ones
round 8 chose for the momentum refresh's block counts (a last round of 0 / 1, 16 / 17 and 5 .. 9 ChaCha blocks): the four-lanes-per-block
form of that round was measured slower and is not in the build (profiles/r08_k2_sampling_epilogue_ab.txt); the cases stay."""
import functools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

N_CHAINS, NUM_TUNE = 6, 20
LAUNCHES = [NUM_TUNE, 30, 30]          # the warm-up, then 60 further draws in two launches
N_DRAWS = sum(LAUNCHES)
DIMS = [(480, 8), (600, 16), (1000, 16), (1024, 16)]


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def make_settings(dim):
    return N.DiagNutsSettings(num_chains=N_CHAINS, seed=800 + dim % 97, num_tune=NUM_TUNE)


@functools.lru_cache(maxsize=None)
def oracle_run(dens, dim):
    from oracle import oracle as O
    s, logp = make_settings(dim), make_logp(dens, dim)
    x0 = O.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    pos, st, _, failed = O.run(oracle_settings(O, s), logp.kind, dim, logp.params, O.gpu_cfg(64), N_CHAINS, x0, N_DRAWS, n_threads=N_CHAINS)
    assert failed == 0
    pos.setflags(write=False)
    st.setflags(write=False)
    return x0, pos, st


@pytest.mark.parametrize("dim,dpl", DIMS, ids=[f"dim{d}" for d, _ in DIMS])
@pytest.mark.parametrize("dens", ["iid", "diag"])
def test_sampling_draws_bit_exact(oracle, dens, dim, dpl):
    x0, pos_o, st_o = oracle_run(dens, dim)
    b = N.ChainBatch(make_settings(dim), make_logp(dens, dim), N_CHAINS)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (dpl, 64)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos, st = [], []
    for k in LAUNCHES:
        p, q = b.draw_many(k)
        pos.append(p)
        st.append(q)
    n_sampling = sampling_launches(b)
    b.close()
    assert n_sampling == 2                  # the two launches after the warm-up ran the sampling build
    pos_g, st_g = np.concatenate(pos), np.concatenate(st)
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    assert (st_g["tuning"][:NUM_TUNE] == 1).all() and (st_g["tuning"][NUM_TUNE:] == 0).all()
