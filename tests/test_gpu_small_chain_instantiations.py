"""Every kernel instantiation of the small-chain families is run against the oracle at least once, on purpose.

`test_gpu_every_instantiation.py` is the per-instantiation guard of the one-chain-per-block family (a miscompile is a
per-instantiation event).  This file is the same guard for the two families that serve "thousands of small chains":

  several chains per wavefront (csrc/nuts_group_impl.hpp): `nuts_group_draw_kernel<Dens, TUNE, ROOMY>` in grp8 / grp16 / grp32
      (density, lanes per chain)  x  {Euclidean, ExactNormal, Microcanonical NUTS, MCLMC}  x  {roomy, non-roomy build}  x  the ends of the size's dims
      The roomy build (one wavefront per SIMD) serves grids of at most 4 x CUs blocks, the non-roomy one (two per SIMD) every larger grid:
      different register allocations of the same source.  Each run asserts from the engine's counter WHICH build served it.
  one chain per lane (csrc/nuts_lane.hpp): `nuts_lane_draw_kernel<Dens | KinWrap<Dens>, NP, TUNE>`
      (density, lane pairs)  x  {Euclidean, ExactNormal, Microcanonical NUTS}  x  the ends of NP's dims

Every run is cut at the end of the warm-up, so the TUNE and the DRAW kernel are both launched.  Inputs are generic doubles (the oracle runs
in the same process on the same arrays).  No case is skipped: the inputs are chosen so that no initial point is rejected (checked with the
oracle alone by tools/small_chain_dry_run.py), and the test asserts it.  The draw every kernel restates: reference src/chain.rs:150-243."""
import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, run_engine, run_oracle

pytestmark = pytest.mark.gpu

# ---- the case list: plain data ---------------------------------------------------------------------------------------------------------------
# lanes per chain -> (first, last) dim it serves (csrc/nuts_contract.hpp group_size), lane pairs -> dims (csrc/nuts_contract.hpp lane_pairs)
GROUP_DIMS = {8: (1, 16), 16: (17, 32), 32: (33, 64)}
LANE_DIMS = {2: (1, 4), 4: (5, 8), 5: (9, 10)}
GROUP_FAMILIES = ("euclid", "exact", "micro", "mclmc")     # MCLMC and the kinds are run-time paths of ONE KinWrap instantiation: a run each
LANE_FAMILIES = ("euclid", "exact", "micro")               # (MCLMC has no one-chain-per-lane form)
GROUP_PAIRS = [(d, g) for d in ("iid", "diag", "funnel", "mvn") for g in (8, 16, 32)] + [("schools", 8)]
LANE_PAIRS = [(d, p) for d in ("iid", "diag", "funnel") for p in (2, 4, 5)] + [("schools", 5)]
STRIDED_DENSITY = "diag"       # per group size and family, one more non-roomy run with about twice as many chains as its grid holds
NUM_TUNE, N_DRAWS, MAXDEPTH = 40, 60, 6
LANE_CHAINS = 70               # one full wavefront and a partial one
ROOMY_CHAINS = 41              # the roomy runs: a few dozen chains, full wavefronts (5 / 10 / 20) and one that holds a single chain
WINDOW = 16                    # chains per oracle window: four windows = 64 chains a run, five in the strided runs
# a case whose default seed (100 + dim) gives the oracle a chain that fails (tools/small_chain_dry_run.py) gets another one here, by id
SEEDS = {}


def group_size(dim):
    return 8 if dim <= 16 else 16 if dim <= 32 else 32 if dim <= 64 else 0


def lane_pairs(dim):
    return 2 if dim <= 4 else 4 if dim <= 8 else 5 if dim <= 10 else 0


def min_dim(dens, fam):
    """The funnel is v plus at least one x; the ESH dynamics (Microcanonical, MCLMC) need two dimensions."""
    return 2 if dens == "funnel" or fam in ("micro", "mclmc") else 1


def _ends(dens, fam, lo, hi):
    if dens == "schools":
        return [10]
    return [max(lo, min_dim(dens, fam)), hi]


def group_cases():
    out = []
    for dens, gs in GROUP_PAIRS:
        for fam in GROUP_FAMILIES:
            ends = _ends(dens, fam, *GROUP_DIMS[gs])
            for dim in ends:                   # the non-roomy build at both ends of the size's range
                out.append(dict(kernel="group", dens=dens, size=gs, fam=fam, build="nonroomy", dim=dim, strided=False))
            out.append(dict(kernel="group", dens=dens, size=gs, fam=fam, build="roomy", dim=ends[-1], strided=False))
            if dens == STRIDED_DENSITY:
                out.append(dict(kernel="group", dens=dens, size=gs, fam=fam, build="nonroomy", dim=ends[-1] - 1, strided=True))
    return out


def lane_cases():
    out = []
    for dens, npairs in LANE_PAIRS:
        for fam in LANE_FAMILIES:
            for dim in _ends(dens, fam, *LANE_DIMS[npairs]):
                out.append(dict(kernel="lane", dens=dens, size=npairs, fam=fam, build="lane", dim=dim, strided=False))
    return out


def case_id(c):
    tag = {"group": "gs", "lane": "np"}[c["kernel"]]
    return f"{c['dens']}-{tag}{c['size']}-{c['fam']}-{c['build']}{'-strided' if c['strided'] else ''}-dim{c['dim']}"


def chain_plan(c, cus):
    """-> (n_chains, grid_blocks, [window offsets]) of a case on a device with `cus` compute units."""
    if c["kernel"] == "lane":
        return LANE_CHAINS, 0, list(range(0, LANE_CHAINS, WINDOW))          # every chain (the last window is clipped)
    gpw = 64 // c["size"]                  # chains per wavefront = per block
    if c["build"] == "roomy":
        return ROOMY_CHAINS, 0, list(range(0, ROOMY_CHAINS, WINDOW))                             # every chain
    if c["strided"]:
        grid = 4 * cus + 2                 # > 4 x CUs: the non-roomy build; the chains need about twice that: the kernel's stride loop runs
        n = (2 * grid - 3) * gpw + 1
        second = grid * gpw - 4            # the last chains of the first pass and the first of the second
        return n, grid, [0, (grid // 2) * gpw - WINDOW // 2, second, second + (grid // 2) * gpw, n - WINDOW]
    blocks = 4 * cus + 4
    n = (blocks - 1) * gpw + 1             # ragged: the last wavefront holds one chain
    return n, 0, [0, (blocks // 2) * gpw - WINDOW // 2, (blocks // 4) * gpw + 1, n - WINDOW]


def make_settings(c, n_chains):
    seed = SEEDS.get(case_id(c), 100 + c["dim"])
    if c["fam"] == "mclmc":
        return N.DiagMclmcSettings(num_chains=n_chains, seed=seed, num_tune=NUM_TUNE, step_size=0.4)
    kind = {"euclid": N.KineticEnergyKind.EUCLIDEAN, "exact": N.KineticEnergyKind.EXACT_NORMAL, "micro": N.KineticEnergyKind.MICROCANONICAL}[c["fam"]]
    return N.DiagNutsSettings(num_chains=n_chains, seed=seed, num_tune=NUM_TUNE, maxdepth=MAXDEPTH, trajectory_kind=kind)


def make_logp(c, seed):
    """Generic doubles, made on the spot."""
    rng = np.random.default_rng(seed)
    dens, dim = c["dens"], c["dim"]
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, float(rng.uniform(-3, 3)))
    if dens == "diag":
        return N.LogpSpec.diag_normal(np.exp(rng.uniform(-3, 3, dim)))
    if dens == "funnel":
        return N.LogpSpec.funnel(dim)
    if dens == "schools":
        return N.LogpSpec.eight_schools()
    a = rng.normal(size=(dim, dim))
    p = a @ a.T / dim + np.eye(dim)
    return N.LogpSpec.mvn_precision((p + p.T) / 2)


def oracle_windows(O, c, s, logp, x0, offsets):
    """The oracle's draws of the chains in the windows: (chain ids, positions, statistics, failed chains)."""
    ids, pos, st, failed = [], [], [], 0
    n = len(x0)
    for off in offsets:
        w = min(WINDOW, n - off)
        p, q, _, f = run_oracle(O, s, logp, w, x0[off:off + w], N_DRAWS, chain_id_offset=off, gpu_threads=64)
        ids.append(np.arange(off, off + w))
        pos.append(p)
        st.append(q)
        failed += f
    return np.concatenate(ids), np.concatenate(pos, axis=1), np.concatenate(st, axis=1), failed


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _run_case(O, c):
    cus = _cus()
    n, grid, offsets = chain_plan(c, cus)
    s = make_settings(c, n)
    logp = make_logp(c, s.seed)
    x0 = O.init_positions_uniform(s.seed, 0, n, c["dim"])
    kw = dict(lane_chains=2) if c["kernel"] == "lane" else dict(lane_groups=2, grid_blocks=grid)
    pos_g, st_g, ex = run_engine(s, logp, n, x0, N_DRAWS, splits=(NUM_TUNE,), **kw)
    assert (ex["status"] == 0).all(), "the engine rejected an initial point"
    assert ex["threads_per_chain"] == 64 and ex["dims_per_lane"] == 2
    # which kernels served: the TUNE and the DRAW kernel of the build the case is written for, and nothing else
    served = (ex["group_launches"], ex["group_roomy_launches"], ex["lane_launches"])
    want = (0, 0, 2) if c["kernel"] == "lane" else (2, 2 if c["build"] == "roomy" else 0, 0)
    assert served == want, f"(group, roomy group, lane) launches {served}, expected {want}; group grid {ex['group_grid']} on {cus} CUs"
    if c["kernel"] == "group":
        need = -(-n // (64 // c["size"]))
        assert (ex["group_grid"] <= 4 * cus) == (c["build"] == "roomy")
        assert (ex["group_grid"] < need) == c["strided"], "the stride loop runs in the strided cases and only there"
    assert (st_g["chain_status"] == 0).all(), "a chain of the engine run failed"
    ids, pos_o, st_o, failed = oracle_windows(O, c, s, logp, x0, offsets)
    assert failed == 0, "an oracle chain failed: pick another seed for this case (SEEDS)"
    assert len(np.unique(ids)) >= (64 if c["kernel"] == "group" and c["build"] == "nonroomy" else n)
    assert_bit_exact(np.ascontiguousarray(pos_g[:, ids]), np.ascontiguousarray(st_g[:, ids]), pos_o, st_o)
    if c["fam"] == "mclmc":
        for f in ("energy_change", "average_step_size"):
            a, b = st_g[f][:, ids], st_o[f]
            assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), f


@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in group_cases()])
def test_group_instantiation_bit_exact(oracle, case):
    _run_case(oracle, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in lane_cases()])
def test_lane_instantiation_bit_exact(oracle, case):
    _run_case(oracle, case)
