"""Shared helpers for the parity tests: run the same configuration on the HIP engine and on the CPU oracle."""
import ctypes as C

import numpy as np

import nuts_rs_amd as N
from nuts_rs_amd import _lib

STAT_FIELDS_EXACT = ["draw", "chain", "depth", "maxdepth_reached", "diverging", "tuning", "n_steps",
                     "index_in_trajectory", "transformation_index", "chain_status", "transformation_update_id"]
STAT_FIELDS_FLOAT = ["step_size", "step_size_bar", "mean_tree_accept", "mean_tree_accept_sym", "max_energy_error",
                     "logp", "energy", "energy_error", "fisher_distance"]


def oracle_settings(O, settings: N.DiagNutsSettings):
    """DiagNutsSettings -> the oracle's Settings struct (same field names)."""
    c = settings.to_c()
    s = O.Settings()
    for name, _ in O.Settings._fields_:
        setattr(s, name, getattr(c, name))
    return s


def group_build_counters(b):
    """(launches of the several-chains-per-wavefront kernels served by the one-wavefront-per-SIMD builds, the grid of those launches):
    debug exports of the library, not part of the ABI, bound here as bench.py and tools/prof_*.py bind theirs."""
    L = N.load_library()
    out = []
    for fn in (L.nm_debug_group_roomy_launches, L.nm_debug_group_grid):
        fn.argtypes, fn.restype = [C.c_void_p], C.c_uint64
        out.append(int(fn(b._h)))
    return tuple(out)


def sampling_launches(b):
    """launches of the sampling-phase build so far: a debug export of the library, not part of the ABI"""
    fn = N.load_library().nm_debug_sampling_launches
    fn.argtypes, fn.restype = [C.c_void_p], C.c_uint64
    return int(fn(b._h))


def run_engine(settings, logp, n_chains, x0, n_draws, chain_id_offset=0, dims_per_lane=0, waves_per_chain=0,
               lane_groups=0, grid_blocks=0, splits=(), lane_chains=0):
    """`splits`: draw counts at which the run is cut into separate launches; the pieces are concatenated."""
    b = N.ChainBatch(settings, logp, n_chains, chain_id_offset=chain_id_offset, dims_per_lane=dims_per_lane,
                     waves_per_chain=waves_per_chain, lane_groups=lane_groups, grid_blocks=grid_blocks, lane_chains=lane_chains)
    status = b.set_position(x0, raise_on_error=False)
    pos, st = None, None
    if (status == 0).all():
        cuts = [0] + [c for c in splits if 0 < c < n_draws] + [n_draws]
        parts = [b.draw_many(hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        pos, st = np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])
    extra = dict(status=status, threads_per_chain=b.threads_per_chain(), dims_per_lane=b.dims_per_lane(),
                 group_launches=b.group_launches(), lane_launches=b.lane_launches())
    extra["group_roomy_launches"], extra["group_grid"] = group_build_counters(b)
    if pos is not None:
        sd, mu = b.mass_matrix()
        extra.update(stds=sd, mean=mu, step_sizes=b.step_sizes(), x=b.positions(), gx=b.gradients(),
                     counters=b.counters())
    b.close()
    return pos, st, extra


def run_oracle(O, settings, logp, n_chains, x0, n_draws, chain_id_offset=0, gpu_threads=64, cfg=None, n_threads=8):
    cfg = cfg or O.gpu_cfg(gpu_threads)
    return O.run(oracle_settings(O, settings), logp.kind, logp.dim, logp.params, cfg, n_chains, x0, n_draws,
                 chain_offset=chain_id_offset, n_threads=n_threads)


def oracle_chains(oracle, s, logp, plan, n_chains, cfg=None):
    """One oracle chain per engine chain, every chain through the same `plan`: a list of steps
      ("set", x[chains][dim])                    set_position of every chain, status 0 expected
      ("set", x[chains][dim], mask)              ... of the chains with mask[c] only (rows of the others are never read)
      ("set", x[chains][dim], mask, expect)      ... with the status expect[c] expected of chain c (None: all chains, 0)
      ("draw", k, ...)                           k draws of every chain whose last set_position succeeded (further entries are the engine's)
    -> positions [draws][chains][dim], statistics [draws][chains], and per step a dict of the chains' state() after it: x, gx, stds, mean
    [chains][dim], step_size [chains], ok [chains] (a chain that is not ok has no state: its rows are NaN, its draws' rows unwritten)."""
    so = oracle_settings(oracle, s)
    cfg = cfg or oracle.gpu_cfg(64)
    n_draws = sum(step[1] for step in plan if step[0] == "draw")
    pos = np.full((n_draws, n_chains, logp.dim), np.nan)
    st = np.zeros((n_draws, n_chains), dtype=oracle.STATS_DTYPE)
    states = [dict(x=np.full((n_chains, logp.dim), np.nan), gx=np.full((n_chains, logp.dim), np.nan), stds=np.full((n_chains, logp.dim), np.nan),
                   mean=np.full((n_chains, logp.dim), np.nan), step_size=np.full(n_chains, np.nan), ok=np.zeros(n_chains, dtype=bool)) for _ in plan]
    for c in range(n_chains):
        ch = oracle.Chain(so, logp.kind, logp.dim, logp.params, cfg, chain_id=c)
        t, ok = 0, False
        for i, step in enumerate(plan):
            if step[0] == "set":
                x, mask, expect = (list(step[1:]) + [None, None])[:3]
                if mask is None or mask[c]:
                    rc = ch.set_position(x[c])
                    assert rc == (0 if expect is None else expect[c]), (i, c, rc)
                    ok = rc == 0
            else:
                for k in range(step[1]):
                    if ok:
                        pos[t + k, c], st[t + k, c], rc = ch.draw()
                        assert rc == 0, (i, c, k, rc)
                t += step[1]
            if ok:
                q = ch.state()
                for f in ("x", "gx", "stds", "mean", "step_size"):
                    states[i][f][c] = q[f]
            states[i]["ok"][c] = ok
    return pos, st, states


def assert_bit_exact(pos_g, st_g, pos_o, st_o):
    """Draw-for-draw, bit-for-bit: positions and every statistic."""
    for f in STAT_FIELDS_EXACT:
        bad = np.argwhere(st_g[f] != st_o[f])
        assert bad.size == 0, f"stat {f} differs first at (draw, chain) = {bad[0]}: gpu {st_g[f][tuple(bad[0])]} oracle {st_o[f][tuple(bad[0])]}"
    for f in STAT_FIELDS_FLOAT + ["divergence_energy_error"]:
        a, b = st_g[f].view(np.uint64), st_o[f].view(np.uint64)
        both_nan = np.isnan(st_g[f]) & np.isnan(st_o[f])
        bad = np.argwhere((a != b) & ~both_nan)
        assert bad.size == 0, f"stat {f} differs first at (draw, chain) = {bad[0]}: gpu {st_g[f][tuple(bad[0])]!r} oracle {st_o[f][tuple(bad[0])]!r}"
    bad = np.argwhere(pos_g.view(np.uint64) != pos_o.view(np.uint64))
    assert bad.size == 0, f"positions differ first at (draw, chain, dim) = {bad[0]}"


def assert_vectors_bit_exact(vec_g, vec_o):
    """Vector-valued statistics: same bits, and the same rows left unwritten (NaN)."""
    assert set(vec_g) <= set(vec_o)
    for k, g in vec_g.items():
        o = vec_o[k]
        both_nan = np.isnan(g) & np.isnan(o)
        bad = np.argwhere((g.view(np.uint64) != o.view(np.uint64)) & ~both_nan)
        assert bad.size == 0, f"{k} differs first at (draw, chain, dim) = {bad[0]}: gpu {g[tuple(bad[0])]!r} oracle {o[tuple(bad[0])]!r}"


# ---- low-rank transformations: inputs and runs shared by tests/test_gpu_lowrank.py, tests/test_gpu_stepsize_protocol.py and tools/ ----
def random_transform(rng, dim, rank, per_chain=0):
    shape = (per_chain,) if per_chain else ()
    stds = np.exp(rng.normal(0, 0.5, shape + (dim,)))
    mean = rng.normal(0, 1, shape + (dim,))
    mu = rng.normal(0, 0.3, shape + (dim,))
    vals = np.exp(rng.uniform(-2, 3, shape + (rank,)))
    if per_chain:
        vecs = np.stack([np.linalg.qr(rng.normal(size=(dim, rank)))[0].T for _ in range(per_chain)])
    else:
        vecs = np.linalg.qr(rng.normal(size=(dim, rank)))[0].T
    return stds, mean, vals, np.ascontiguousarray(vecs), mu


def correlated_precision(rng, dim, rank, scale=50.0):
    u = np.linalg.qr(rng.normal(size=(dim, rank)))[0]
    sigma = np.eye(dim) + u @ np.diag(rng.uniform(5.0, scale, rank)) @ u.T
    sc = np.exp(rng.normal(0, 0.5, dim))
    sigma = np.diag(sc) @ sigma @ np.diag(sc)
    prec = np.linalg.inv(sigma)
    return (prec + prec.T) / 2, sigma


def run_fixed(oracle, logp, settings, n_chains, transform, n_draws, waves_per_chain=0, dims_per_lane=0, chain_tiles=0,
              expect_tiles=None, splits=(), expect_order=None):
    x0 = oracle.init_positions_uniform(settings.seed, 0, n_chains, logp.dim)
    b = N.ChainBatch(settings, logp, n_chains, waves_per_chain=waves_per_chain, dims_per_lane=dims_per_lane, chain_tiles=chain_tiles)
    assert (b.set_position(x0) == 0).all()
    b.set_transform(*transform)
    cuts = [0] + [c for c in splits if 0 < c < n_draws] + [n_draws]
    parts = [b.draw_many(hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    pos, st = np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])
    tpc = b.threads_per_chain()
    tiles = b.tile_launches() > 0              # the matrix-core kernels sum U'v sequentially: the oracle's lr_seq_dots mode
    order = b.reduce_order()                   # (1: the tile kernel, 2: the lockstep kernel with its own order of the sums over dim)
    if expect_tiles is not None:
        assert tiles == expect_tiles
    if expect_order is not None:
        assert order == expect_order
    assert (order > 0) == tiles and (order == 2) == (b.lockstep_launches() > 0)
    b.close()
    pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, settings), logp.kind, logp.dim, logp.params,
                                        oracle.gpu_cfg(tpc, lr_seq_dots=order), n_chains, x0, n_draws, n_threads=8, transform=transform)
    assert failed == 0
    return pos, st, pos_o, st_o


def estimator_pair(oracle):
    """the oracle's LAPACK estimator, as a callback for the oracle and as a callback for the engine (same function)"""
    from oracle import lowrank as LR
    rec = []
    cb_o = LR.estimator_callback(rec)
    cb_e = C.cast(cb_o, _lib.LOWRANK_ESTIMATOR_FN)
    return cb_o, cb_e, rec
