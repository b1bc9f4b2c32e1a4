"""`Chain::set_position` in the middle of a run and for some chains only (`ChainBatch.set_position(mask=...)`), on every kernel family.

The engine decides on the host which kernels serve a draw call (nuts_engine.hip: `draws_launched` = the draw index of the healthy chain that
is furthest behind, `sampling_from`, the tune / draw forms of the several-chains-per-wavefront and one-chain-per-lane kernels, the
matrix-core tile kernel's own branch), every family is initialised by the wave family's K_INIT (in cluster mode by its own masked loop),
and the sampling build leaves x / g_x stale in memory between the draws of a launch.  A mistake in any of these gives plausible draws with
wrong bits.  Here the engine and one `oracle.Chain` per engine chain perform the same sequence of set_position and draw calls:

  positions and every statistics field of every draw are the oracle's bits (helpers.assert_bit_exact), and after EVERY step of the plan
  positions(), gradients(), step_sizes() and mass_matrix() are the bits of the oracle chains' state() (x, gx, step_size, stds, mean);
  the draw index keeps counting across set_position; a re-set chain reports its new transformation on its next draw and nobody else does;
  the launch counters show which family, and on the sampling-build cases which build, served each call.

The plan (num_tune = 12; x0, x1 from init_positions_uniform(seed, ...), (seed + 1, ...)): set_position(x0) of all chains; 5 draws; a masked
set_position inside the warm-up (chain 1, and one chain of the last wavefront / tile), the rows of the other chains NaN; 11 draws in one
call, across draw index num_tune; in the sampling phase a masked set_position of the next chains (2, ...), on the iid normal first to the
density's mean (zero gradient: status 1, the oracle chain's too), then to x1; 6 draws, as one call and as calls of 1 and 5; set_position(x1)
of all chains; 3 draws.  test_late_starter_masked: a chain whose first point is rejected joins, by a masked set_position, when the others
are past their warm-up.

MclmcChain keeps the same state in the oracle (position, gradient, diagonal mass matrix, fixed step size), so state() has an equivalent
for everything that is read back and the MCLMC case compares all of it too, with its two extra statistics.

Not covered here: LowRankNutsSettings / LowRankMclmcSettings engines (oracle.Chain has no Python-level transformation or estimator
plumbing; the reference's deque semantics on a retry are pinned in test_gpu_lowrank.py), host-callback and module densities.

`python tests/test_gpu_chain_lifecycle.py --dry-run` runs every case's plan on the oracle alone (no GPU) and checks that the plans are
sound: no oracle chain fails, every bad point is rejected, the transformation report and the draw indices are as the tests expect."""
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_chains, sampling_launches

pytestmark = pytest.mark.gpu

NUM_TUNE = 12
EXACT, MICRO = N.KineticEnergyKind.EXACT_NORMAL, N.KineticEnergyKind.MICROCANONICAL
WAVE1 = dict(lane_groups=1, lane_chains=1, chain_tiles=1)

# name -> (family, sampler, density, dim, chains, chains re-set inside the warm-up (the next ones are re-set in the sampling phase),
#          ChainBatch arguments, (dims_per_lane, threads_per_chain) or None)
CASES = {}


def _case(name, family, dens, dim, n, masked, engine, tiling=None, sampler="nuts"):
    CASES[name] = (family, sampler, dens, dim, n, masked, engine, tiling)


# one wavefront (or two) per chain, tilings without a sampling build
_case("wave_2x1_iid100", "wave", "iid", 100, 4, (1,), dict(WAVE1, dims_per_lane=2, waves_per_chain=1), (2, 64))
_case("wave_4x1_funnel130", "wave", "funnel", 130, 4, (1,), dict(WAVE1, dims_per_lane=4, waves_per_chain=1), (4, 64))
_case("wave_8x2_diag700", "wave", "diag", 700, 4, (1,), dict(WAVE1, dims_per_lane=8, waves_per_chain=2), (8, 128))
# ... with the sampling build: the bottom of the (8, 1) and of the (16, 1) tiling
for _dens in ("iid", "diag", "funnel", "mvn"):
    _case(f"sampling_8x1_{_dens}257", "sampling", _dens, 257, 4, (1,), {}, (8, 64))
    _case(f"sampling_16x1_{_dens}513", "sampling", _dens, 513, 4, (1,), {}, (16, 64))
# 8 / 4 / 2 chains per wavefront: the re-set chains share their wavefronts with untouched ones, the last wavefront is partial
_case("group_iid8", "group", "iid", 8, 19, (1, 9), dict(lane_groups=2, lane_chains=1))
_case("group_funnel20", "group", "funnel", 20, 19, (1, 9), dict(lane_groups=2, lane_chains=1))
_case("group_diag40", "group", "diag", 40, 19, (1, 9), dict(lane_groups=2, lane_chains=1))
# one chain per lane: 64 chains per wavefront, the second wavefront has 6
_case("lane_schools10", "lane", "schools", 10, 70, (1, 65), dict(lane_chains=2))
_case("lane_iid8", "lane", "iid", 8, 70, (1, 65), dict(lane_chains=2))
_case("lane_diag10", "lane", "diag", 10, 70, (1, 65), dict(lane_chains=2))
# ... requested at dim 11 .. 16, where no one-chain-per-lane kernel exists any more (test_gpu_lane_chains.py::test_removed_lane_forms): the
# engine's choice for 70 chains of these dims is the wave kernels on the (2, 1) tiling, and the counters say so
_case("lane_request_iid12", "wave", "iid", 12, 70, (1, 65), dict(lane_chains=2), (2, 64))
_case("lane_request_diag16", "wave", "diag", 16, 70, (1, 65), dict(lane_chains=2), (2, 64))
# the matrix-core tile kernel with the diagonal adaptation: 16 chains per tile, the second tile has 4
_case("tile_mvn64", "tile", "mvn", 64, 20, (1, 17), dict(chain_tiles=2, lane_groups=1))
_case("tile_mvn100_padded", "tile", "mvn", 100, 20, (1, 17), dict(chain_tiles=2, lane_groups=1))
# two blocks per chain: K_INIT's own masked loop in cluster mode
_case("cluster_diag4500", "cluster", "diag", 4500, 3, (1,), {}, (16, 256))
# the other integrators
_case("exact_wave_iid300", "wave", "iid", 300, 4, (1,), dict(lane_groups=1, lane_chains=1), sampler=EXACT)
_case("micro_wave_iid300", "wave", "iid", 300, 4, (1,), dict(lane_groups=1, lane_chains=1), sampler=MICRO)
_case("exact_lane_iid10", "lane", "iid", 10, 70, (1, 65), dict(lane_chains=2), sampler=EXACT)         # (launch_lane_kin)
_case("micro_lane_iid10", "lane", "iid", 10, 70, (1, 65), dict(lane_chains=2), sampler=MICRO)
_case("exact_lane_request_iid12", "wave", "iid", 12, 70, (1, 65), dict(lane_chains=2), (2, 64), sampler=EXACT)
_case("micro_lane_request_iid12", "wave", "iid", 12, 70, (1, 65), dict(lane_chains=2), (2, 64), sampler=MICRO)
_case("mclmc_wave_diag50", "wave", "diag", 50, 4, (1,), dict(lane_groups=1), sampler="mclmc")

LATE_CASES = ["sampling_16x1_iid513", "lane_iid8", "lane_request_iid12", "tile_mvn64"]
LATE_CHAIN = 2
STEP6 = {"one_call": [6], "calls_1_5": [1, 5]}


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    if dens == "funnel":
        return N.LogpSpec.funnel(dim)
    if dens == "schools":
        return N.LogpSpec.eight_schools()
    rng = np.random.default_rng(dim)
    if dens == "mvn":
        a = rng.normal(size=(dim, dim))
        p = a @ a.T / dim + np.eye(dim)
        return N.LogpSpec.mvn_precision((p + p.T) / 2)
    return N.LogpSpec.diag_normal(np.exp(rng.uniform(-2, 2, dim)))


def make_settings(name):
    _, sampler, _, dim, n, *_ = CASES[name]
    kw = dict(num_chains=n, seed=700 + dim % 89, num_tune=NUM_TUNE)
    if sampler == "mclmc":
        return N.DiagMclmcSettings(**kw)
    return N.DiagNutsSettings(trajectory_kind=0 if sampler == "nuts" else sampler, **kw)


def oracle_cfg(O, name):
    family, tiling = CASES[name][0], CASES[name][7]
    if family == "cluster":
        return O.gpu_cfg(256, gpu_slice=4096)
    return O.gpu_cfg(tiling[1] if tiling else 64)


def only(x, chains):
    """(x with the rows of every other chain NaN: a masked set_position must not read them, the mask)"""
    out = np.full_like(x, np.nan)
    mask = np.zeros(len(x), dtype=bool)
    for c in chains:
        out[c] = x[c]
        mask[c] = True
    return out, mask


def lifecycle_plan(O, name):
    """The plan of the module docstring as oracle_chains takes it (the chains re-set in the sampling phase are returned with it)."""
    _, _, dens, dim, n, masked, _, _ = CASES[name]
    s = make_settings(name)
    x0, x1 = O.init_positions_uniform(s.seed, 0, n, dim), O.init_positions_uniform(s.seed + 1, 0, n, dim)
    later = tuple(c + 1 for c in masked)
    plan = [("set", x0), ("draw", 5),
            ("set", *only(x1, masked)),                       # inside the warm-up
            ("draw", 11)]                                     # draws 5 .. 15: across num_tune = 12
    if dens == "iid":                                         # the density's mean: a zero gradient, BadInitGrad
        expect = np.zeros(n, dtype=np.uint64)
        expect[list(later)] = 1
        plan.append(("set", *only(np.full((n, dim), 3.0), later), expect))
    plan += [("set", *only(x1, later)),                       # in the sampling phase
             ("draw", 6),                                     # (cut into the calls of STEP6 on the engine)
             ("set", x1), ("draw", 3)]
    return plan, later


def late_plan(O, name):
    _, _, dens, dim, n, *_ = CASES[name]
    s = make_settings(name)
    x0 = O.init_positions_uniform(s.seed, 0, n, dim)
    bad = x0.copy()
    bad[LATE_CHAIN] = 3.0 if dens == "iid" else np.nan
    expect = np.zeros(n, dtype=np.uint64)
    expect[LATE_CHAIN] = 1
    return [("set", bad, None, expect), ("draw", NUM_TUNE + 5), ("set", *only(x0, [LATE_CHAIN])), ("draw", NUM_TUNE), ("draw", 8)]


@functools.lru_cache(maxsize=None)
def oracle_reference(name, which):
    """one oracle run per (case, plan), shared by the parametrisations of step 6"""
    from oracle import oracle as O
    plan, later = lifecycle_plan(O, name) if which == "lifecycle" else (late_plan(O, name), None)
    pos, st, states = oracle_chains(O, make_settings(name), make_logp(CASES[name][2], CASES[name][3]), plan, CASES[name][4], oracle_cfg(O, name))
    pos.setflags(write=False)
    st.setflags(write=False)
    return plan, later, pos, st, states


def check_plan_on_oracle(name, which):
    """What the GPU tests take for granted about a plan, on the oracle alone."""
    plan, later, pos, st, states = oracle_reference(name, which)
    n = CASES[name][4]
    for i, step in enumerate(plan):
        if step[0] == "set" and len(step) == 4:               # a bad point is rejected (oracle_chains asserts the status) and nothing else is;
            assert (states[i]["ok"] == (step[3] == 0)).all(), (name, i)
        elif step[0] == "set":                                 # after any other set_position every chain is at work
            assert states[i]["ok"].all(), (name, i)
        else:                                                  # and no chain fails in a draw (oracle_chains asserts every draw's status)
            assert (states[i]["ok"] == states[i - 1]["ok"]).all(), (name, i)
    assert (st["chain_status"] == 0).all()
    if which == "lifecycle":
        assert states[-1]["ok"].all()
        assert (st["draw"] == np.arange(len(st))[:, None]).all()
        first = 16                                             # the first draw after the sampling-phase set_position
        tid = st["transformation_update_id"][first]
        assert (tid[list(later)] >= 0).all() and (np.delete(tid, list(later)) == -1).all() and tid[0] == -1, (name, tid)
    else:
        k = NUM_TUNE + 5
        others = np.arange(n) != LATE_CHAIN
        assert (st["draw"][:, others] == np.arange(len(st))[:, None]).all()
        assert (st["draw"][k:, LATE_CHAIN] == np.arange(len(st) - k)).all()


def dry_run():
    import time
    for which, names in (("lifecycle", list(CASES)), ("late", LATE_CASES)):
        for name in names:
            t0 = time.perf_counter()
            check_plan_on_oracle(name, which)
            print(f"{which:9s} {name:24s} ok  {time.perf_counter() - t0:5.2f} s")


class Engine:
    """A ChainBatch of a case, with the counters that say which kernels served a call."""

    def __init__(self, name):
        family, _, dens, dim, n, _, kw, tiling = CASES[name]
        self.family, self.n = family, n
        self.b = N.ChainBatch(make_settings(name), make_logp(dens, dim), n, **kw)
        if tiling:
            assert (self.b.dims_per_lane(), self.b.threads_per_chain()) == tiling
        assert (self.b.blocks_per_chain() > 1) == (family == "cluster")
        self.count = np.zeros(n, dtype=np.int64)               # draw index of every chain
        self.ok = np.zeros(n, dtype=bool)
        self.sampling_from = NUM_TUNE + 1

    def counters(self):
        b = self.b
        return dict(group=b.group_launches(), lane=b.lane_launches(), tile=b.tile_launches(), sampling=sampling_launches(b),
                    kernel=b.counters()["kernel_launches"])

    def set(self, x, mask=None, expect=None):
        status = self.b.set_position(x.copy(), raise_on_error=False, mask=mask)
        assert (status == (0 if expect is None else expect)).all(), status
        m = np.ones(self.n, dtype=bool) if mask is None else mask
        self.ok[m] = status[m] == 0
        # one general draw first for everybody, from the draw index of the healthy chain that is furthest behind
        self.sampling_from = max(NUM_TUNE, int(self.count[self.ok].min())) + 1

    def draw(self, k):
        before = self.counters()
        lo = int(self.count[self.ok].min())
        pos, st = self.b.draw_many(k, raise_on_error=False)
        d = {f: v - before[f] for f, v in self.counters().items()}
        own = {"wave": "kernel", "sampling": "kernel", "cluster": "kernel"}.get(self.family, self.family)
        assert d[own] == 1, d                                  # the family's counter rises on every call ...
        assert all(d[f] == 0 for f in ("group", "lane", "tile") if f != own), d      # ... and no other family's
        assert d["sampling"] == (1 if self.family == "sampling" and lo + k - 1 >= self.sampling_from else 0), (d, lo, k, self.sampling_from)
        self.count[self.ok] += k
        return pos, st

    def assert_state(self, want, step):
        b = self.b
        ok = want["ok"]
        assert (ok == self.ok).all(), step
        sd, mu = b.mass_matrix()
        for f, got in (("x", b.positions()), ("gx", b.gradients()), ("stds", sd), ("mean", mu), ("step_size", b.step_sizes())):
            bad = np.argwhere(got[ok].view(np.uint64) != want[f][ok].view(np.uint64))
            assert bad.size == 0, f"after step {step}: {f} of the engine differs from the oracle chain's first at (healthy chain, dim) = {bad[0]}"

    def run(self, plan, calls):
        """`plan` on the engine, draw step i in the calls calls.get(i); the state after every step against `states`"""
        pos, st = [], []
        for i, step in enumerate(plan):
            if step[0] == "set":
                self.set(*step[1:])
            else:
                for k in calls.get(i, [step[1]]):
                    p, q = self.draw(k)
                    pos.append(p)
                    st.append(q)
            yield i
        self.pos, self.st = np.concatenate(pos), np.concatenate(st)


def assert_extra_statistics(name, st_g, st_o, rows=slice(None)):
    if CASES[name][1] == "mclmc":
        for f in ("energy_change", "average_step_size"):
            a, b = st_g[f][rows], st_o[f][rows]
            assert ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all(), f


@pytest.mark.parametrize("step6", list(STEP6))
@pytest.mark.parametrize("name", list(CASES))
def test_set_position_mid_run_and_per_chain(oracle, name, step6):
    plan, later, pos_o, st_o, states = oracle_reference(name, "lifecycle")
    i6 = len(plan) - 3
    e = Engine(name)
    try:
        for i in e.run(plan, {i6: STEP6[step6]}):
            e.assert_state(states[i], i)
        total = e.counters()
    finally:
        e.b.close()
    assert_bit_exact(e.pos, e.st, pos_o, st_o)
    assert_extra_statistics(name, e.st, st_o)
    assert (e.st["draw"] == np.arange(len(e.st))[:, None]).all()           # set_position does not reset the chain's draw index
    assert (e.st["chain"] == np.arange(e.n)).all() and (e.st["chain_status"] == 0).all()
    assert (e.st["tuning"][:NUM_TUNE] == 1).all() and (e.st["tuning"][NUM_TUNE:] == 0).all()
    tid = e.st["transformation_update_id"][16]                              # the first draw after the sampling-phase set_position
    assert (tid[list(later)] >= 0).all() and (np.delete(tid, list(later)) == -1).all()
    if e.family != "sampling":
        assert total["sampling"] == 0


@pytest.mark.parametrize("name", LATE_CASES)
def test_late_starter_masked(oracle, name):
    """A chain whose first point is rejected starts its warm-up, by a masked set_position, when the others are sampling: the launches take
    the kernels of the chain that is furthest behind (no sampling build until it is past num_tune), it tunes for its own first num_tune
    draws, and the others continue bit for bit.  The rows of the failed chain before its revival are unwritten and not compared."""
    plan, _, pos_o, st_o, states = oracle_reference(name, "late")
    e = Engine(name)
    try:
        for i in e.run(plan, {}):
            e.assert_state(states[i], i)
    finally:
        e.b.close()
    k = NUM_TUNE + 5
    others = np.arange(e.n) != LATE_CHAIN
    assert_bit_exact(e.pos[:, others], e.st[:, others], pos_o[:, others], st_o[:, others])
    assert_bit_exact(e.pos[k:], e.st[k:], pos_o[k:], st_o[k:])
    late = e.st[k:, LATE_CHAIN]
    assert (late["draw"] == np.arange(NUM_TUNE + 8)).all()
    assert (late["tuning"][:NUM_TUNE] == 1).all() and (late["tuning"][NUM_TUNE:] == 0).all()
    assert (e.st["tuning"][k:, others] == 0).all() and (e.st["draw"][:, others] == np.arange(len(e.st))[:, None]).all()


if __name__ == "__main__":
    if sys.argv[1:] != ["--dry-run"]:
        sys.exit("usage: python tests/test_gpu_chain_lifecycle.py --dry-run")
    dry_run()
