"""Round 9 on the sampling-phase build (nuts_kernels.hpp `SAMPLING`, the one-wavefront tiling of 16 doubles per lane): the rows of a U-turn
test's scratch slots roll through their landing registers (row m computed, row m + 4 requested; level >= 3 tests: m + 2).  Engine against
oracle, bit for bit on positions and every statistics field, on runs whose sampling draws reach what the K2-like cases of
test_gpu_sampling_epilogue.py never do (complete depth-4 trees only): tests of level 3 .. 5 (depth 5 and 6 trees), doublings that a test
below the top ends, on the elementwise and the non-elementwise (funnel) path, and a partly filled tile (dim 600).  Each case first checks on
the oracle's own statistics that its sampling draws still have that coverage."""
import functools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

NUM_TUNE = 20
LAUNCHES = [NUM_TUNE, 20, 20]          # the warm-up, then 40 further draws in two launches
N_DRAWS = sum(LAUNCHES)

# name -> (density, dim, chains, target_accept, maxdepth, coverage its sampling draws must have)
CASES = {
    "iid_ta95": ("iid", 1024, 6, 0.95, 10, "deep"),
    "funnel_md7": ("funnel", 1024, 6, 0.8, 7, "early"),
    "iid_ta30": ("iid", 1024, 8, 0.3, 10, "early"),
    "diag600_ta95": ("diag", 600, 6, 0.95, 10, "deep"),
}


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    if dens == "funnel":
        return N.LogpSpec.funnel(dim)
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def make_settings(name):
    _, dim, n_chains, target_accept, maxdepth, _ = CASES[name]
    s = N.DiagNutsSettings(num_chains=n_chains, seed=900 + dim % 97, num_tune=NUM_TUNE, maxdepth=maxdepth)
    s.adapt_options.step_size_settings.target_accept = target_accept
    return s


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    from oracle import oracle as O
    dens, dim, n_chains = CASES[name][:3]
    s, logp = make_settings(name), make_logp(dens, dim)
    x0 = O.init_positions_uniform(s.seed, 0, n_chains, dim)
    pos, st, _, failed = O.run(oracle_settings(O, s), logp.kind, dim, logp.params, O.gpu_cfg(64), n_chains, x0, N_DRAWS, n_threads=n_chains)
    assert failed == 0
    pos.setflags(write=False)
    st.setflags(write=False)
    return x0, pos, st


def coverage(st):
    """(sampling draws of depth >= 5, non-diverging sampling draws whose last doubling a test below the top ended) in the oracle's statistics."""
    q = st[NUM_TUNE + 1:]
    deep = int((q["depth"] >= 5).sum())
    early = int(((q["diverging"] == 0) & (q["n_steps"] + 1 != 2 ** q["depth"])).sum())
    return deep, early


@pytest.mark.parametrize("name", list(CASES))
def test_sampling_draws_bit_exact(oracle, name):
    dens, dim, n_chains, _, _, want = CASES[name]
    x0, pos_o, st_o = oracle_run(name)
    deep, early = coverage(st_o)
    print(f"{name}: sampling draws of depth >= 5: {deep}, ended below the top without a divergence: {early}, "
          f"depths {np.bincount(st_o['depth'][NUM_TUNE + 1:].ravel().astype(np.int64)).tolist()}")
    assert (deep if want == "deep" else early) > 0, f"{name} lost its coverage ({want}): lengthen the case"
    b = N.ChainBatch(make_settings(name), make_logp(dens, dim), n_chains)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (16, 64)
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


def test_cases_cover_deep_trees_and_early_endings(oracle):
    """Taken together: a sampling draw of depth >= 5, and a non-diverging sampling draw with n_steps + 1 != 2 ** depth."""
    cov = [coverage(oracle_run(name)[2]) for name in CASES]
    assert sum(d for d, _ in cov) > 0 and sum(e for _, e in cov) > 0, cov
