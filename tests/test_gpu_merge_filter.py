"""Round 10 on the sampling-phase build (nuts_kernels.hpp `SAMPLING`, dev_math.hpp merge_filter): its merges are decided on an approximate
log-size, and an undecided one (and one in 256 whatever the filter says) is redone exactly from the wave's log of leaf weights.  Engine against
oracle, bit for bit on positions and every statistics field, on runs whose sampling draws are the K2 tree (depth 4), shallow trees with
weights far apart (target_accept 0.3), deep trees (depth 7: log indices beyond 64), the (8, 1) tiling, extra doublings, doublings a test
below the top ends (their leaves are overwritten in the log), the funnel (with its default energy limit, and with one that makes sampling draws
diverge), a partly filled tile and the full-precision normal.  Each case first checks that the oracle's sampling draws are still the ones
recorded when it was fixed (draws per depth, doublings ended below the top, divergences), and afterwards what
nm_debug_merge_exact_paths counted: the exact path ran (the forced share), and where the filter should decide nearly everything it did."""
import ctypes as C
import functools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

NUM_TUNE = 20
LAUNCHES = [NUM_TUNE, 20, 20]          # the warm-up, then 40 further draws in two launches
N_DRAWS = sum(LAUNCHES)
FORCED = 1.0 / 256.0                   # dev_math.hpp NM_MF_FORCE_BITS = 8

# name -> (density, dim, chains, target_accept, maxdepth, extra_doublings, tiling, what the counter must show,
#          the oracle's sampling draws as recorded when the case was fixed: {depth: draws}, draws a test below the top ended, diverging draws)
CASES = {
    "iid_ta80": ("iid", 1024, 6, 0.8, 10, 0, 16, "decides", {4: 234}, 0, 0),                            # the K2 tree
    "iid_ta30": ("iid", 1024, 8, 0.3, 10, 0, 16, "above_forced", {2: 93, 3: 219}, 15, 0),               # weights far apart (energy errors up to 4.8 in the sampling draws)
    "iid_ta99": ("iid", 1024, 6, 0.99, 10, 0, 16, None, {5: 8, 6: 109, 7: 117}, 0, 0),                  # 127 leaves: log indices beyond 64
    "iid480_ta95": ("iid", 480, 6, 0.95, 10, 0, 8, None, {4: 14, 5: 200, 6: 20}, 0, 0),                 # the (8, 1) tiling
    "iid_md8_x2_ta80": ("iid", 1024, 6, 0.8, 8, 2, 16, None, {6: 234}, 0, 0),                           # 4 + 2 extra doublings
    "iid_md8_x2_ta30": ("iid", 1024, 8, 0.3, 8, 2, 16, "above_forced", {4: 181, 5: 131}, 34, 0),        # discarded doublings overwritten in the log
    "funnel_md7": ("funnel", 1024, 6, 0.8, 7, 0, 16, None, {4: 234}, 2, 0),                             # the non-elementwise path (no divergence after the warm-up)
    "funnel_md7_mee1": ("funnel", 1024, 6, 0.8, 7, 0, 16, None, {1: 3, 2: 11, 3: 3, 4: 131, 5: 86}, 4, 18),   # ... with max_energy_error 1.0: divergences
    "diag600_ta95": ("diag", 600, 6, 0.95, 10, 0, 16, None, {5: 231, 6: 3}, 0, 0),                      # a partly filled tile
    "mvn300": ("mvn", 300, 6, 0.8, 10, 0, 8, None, {4: 234}, 0, 0),                                     # the full-precision normal on its (8, 1) sampling build
}


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    if dens == "funnel":
        return N.LogpSpec.funnel(dim)
    if dens == "diag":
        return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))
    a = np.random.default_rng(dim).normal(size=(dim, dim))
    p = a @ a.T / dim + np.eye(dim)
    return N.LogpSpec.mvn_precision((p + p.T) / 2)


def make_settings(name):
    _, dim, n_chains, target_accept, maxdepth, extra = CASES[name][:6]
    s = N.DiagNutsSettings(num_chains=n_chains, seed=1000 + dim % 97, num_tune=NUM_TUNE, maxdepth=maxdepth, extra_doublings=extra)
    s.adapt_options.step_size_settings.target_accept = target_accept
    if name == "funnel_md7_mee1":
        s.max_energy_error = 1.0        # with the default limit of 1000 the funnel's 40 sampling draws have no divergence; with this one 18 have
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
    """({depth: draws}, draws a test below the top ended, diverging draws) of the sampling draws in the oracle's statistics"""
    q = st[NUM_TUNE + 1:]
    depth = q["depth"].ravel().astype(np.int64)
    early = int(((q["diverging"] == 0) & (q["n_steps"] + 1 != 2 ** q["depth"])).sum())
    return {int(d): int(n) for d, n in enumerate(np.bincount(depth)) if n}, early, int(q["diverging"].sum())


def merge_exact_paths(b):
    """merges of the sampling build that took the exact path so far: a debug export of the library, not part of the ABI"""
    fn = N.load_library().nm_debug_merge_exact_paths
    fn.argtypes, fn.restype = [C.c_void_p], C.c_uint64
    return int(fn(b._h))


@pytest.mark.parametrize("name", list(CASES))
def test_sampling_draws_bit_exact_and_exact_path_counted(oracle, name):
    dens, dim, n_chains, _, _, _, dpl, counter = CASES[name][:8]
    x0, pos_o, st_o = oracle_run(name)
    print(f"{name}: sampling draws by depth, ended below the top, diverging: {coverage(st_o)}; max energy error {float(st_o['max_energy_error'][NUM_TUNE + 1:].max()):.3g}")
    assert coverage(st_o) == CASES[name][8:], f"{name} no longer has the sampling draws it was fixed with"
    b = N.ChainBatch(make_settings(name), make_logp(dens, dim), n_chains)
    assert (b.dims_per_lane(), b.threads_per_chain()) == (dpl, 64)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos, st = [], []
    for k in LAUNCHES:
        p, s_ = b.draw_many(k)
        pos.append(p)
        st.append(s_)
    n_sampling = sampling_launches(b)
    n_exact = merge_exact_paths(b)
    b.close()
    assert n_sampling == 2                  # the two launches after the warm-up ran the sampling build
    pos_g, st_g = np.concatenate(pos), np.concatenate(st)
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
    # one merge per leaf of a doubling that ran to its end: the sampling build's draws made about sum(n_steps) merges (draw NUM_TUNE is the general kernel's)
    steps = int(st_g["n_steps"][NUM_TUNE + 1:].sum())
    print(f"{name}: {n_exact} exact-path merges, {steps} leapfrogs in the sampling build's draws ({n_exact / steps:.4f})")
    assert n_exact > 0
    if counter == "decides":
        assert n_exact <= 0.02 * steps
    if counter == "above_forced":
        assert n_exact > FORCED * steps


def test_filter_is_left_out_beyond_its_depth_bound(oracle):
    """maxdepth + extra_doublings beyond what the filter's error bound covers (dev_math.hpp NM_MF_MAX_MD = 12): the engine stays on the general kernel."""
    s = N.DiagNutsSettings(num_chains=2, seed=5, num_tune=4, maxdepth=13)
    logp = N.LogpSpec.iid_normal(1024, 3.0)
    b = N.ChainBatch(s, logp, 2)
    from oracle import oracle as O
    x0 = O.init_positions_uniform(s.seed, 0, 2, 1024)
    assert (b.set_position(x0, raise_on_error=False) == 0).all()
    pos_g, st_g = b.draw_many(8)
    n_sampling, n_exact = sampling_launches(b), merge_exact_paths(b)
    b.close()
    assert (n_sampling, n_exact) == (0, 0)
    pos_o, st_o, _, failed = O.run(oracle_settings(O, s), logp.kind, 1024, logp.params, O.gpu_cfg(64), 2, x0, 8, n_threads=2)
    assert failed == 0
    assert_bit_exact(pos_g, st_g, pos_o, st_o)
