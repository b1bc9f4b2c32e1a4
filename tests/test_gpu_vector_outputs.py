"""The nine vector-valued outputs of `nm_draw_outputs` — `Chain::expanded_draw`'s half of the drop-in boundary (reference src/chain.rs:190-204) —
on every kernel family, bit for bit against the oracle's copies of the same reference fields.

Every family writes these rows with its own store code: `write_row`'s masked loop with the block's slice offset (csrc/nuts_kernels.hpp),
`emit_divergence_vectors` with its two arms (a divergent leapfrog that started at the trajectory's initial point reads x / g_x from the chain's
persistent slots, any other start point is rebuilt from its stashed z and the density is evaluated again), the `st_nat` stores of the lockstep
matrix-core kernel (csrc/nuts_lockstep.hpp), the tile kernel's, the group and lane kernels' own `P.out_*` sites.  The parity suites compare
positions and scalar statistics everywhere and the vectors in a few Euclidean cases; here every family is asked for ALL its vectors:

  A  one-chain kernels, Euclidean NUTS, DiagNutsSettings: the eight tilings, each at a ragged odd dim and at its full tile (index-dependent
     diagonal normal, max_energy_error 0.25 — the parity test's device for forcing divergences); the funnel on (2,1) and (4,1); the
     full-precision normal with chain_tiles = 1 on (4,1)
  B  the low-rank transformation: adapting (default tiling, two wavefronts at dim 300), a frozen shared transformation on the full-precision
     normal on the tile kernel (chain_tiles = 2, and the automatic choice of settings with store_divergences) and on the lockstep kernel
     (chain_tiles = 3), a per-chain frozen transformation on a wave kernel
  C  ExactNormal, Microcanonical, MCLMC (KinWrap) on (16,1) ragged and (4,4); the (16,1) MCLMC case runs the step-halving ladder
  D  chains wider than one block: dim 4097 (a second slice of ONE element) and 8193 (three blocks), iid and diagonal normal, every kind at
     4097, NM_CLUSTER_GENERAL=1 once at 8193
  E  the host callback: HostCb on (2,1), (4,4), ragged (16,4); LrWrap<HostCb>, KinWrap<HostCb>, a wide chain; two cases with recoverable errors
  F  the group kernels (8 / 4 / 2 chains per wavefront) and the lane kernels under ExactNormal, Microcanonical, MCLMC
  G  one vector requested alone (the kernels branch on the individual pointers), and the device path with sentinel-filled buffers

Refused (asserted with status and text, not run): the lockstep kernel writes no divergence / mass-matrix vectors — a draw call that asks it
for one is NM_ERR_UNSUPPORTED with `lockstep_outputs_error`'s text, for chain_tiles = 0 and 3 (test_lockstep_refuses_event_vectors).  The
one-chain-per-lane kernels have no MCLMC form (`plan_engine`: lane_kin_ok), so F's lane cases are ExactNormal and Microcanonical.

Every case asserts which kernel served it, runs two launches cut at an odd draw count, and asserts on the engine's own statistics — shown
equal to the oracle's first — that the events it is about occur (CONDITIONS below).  Seeds are chosen with the oracle alone:
`python tools/small_chain_dry_run.py --only vectors` scans seeds 0 .. 31 per case and prints the first that meets the case's conditions; the
lists here carry those seeds, and the tool reports nothing for them.  The inputs are built from exact operations only (dyadic numbers,
+-1/2 eigenvectors, integer matrices): the oracle's draws, and with them the seeds, do not depend on a machine's libm or LAPACK.  The host
callback's density is the plain-numpy one of tests/test_gpu_host_callback_instantiations.py.

Conditions a case drops, by construction: a frozen transformation has no mass-matrix event after draw 0 ("mm"); the lockstep kernel writes
no divergence vectors ("div0", "divN"); MCLMC has no chosen point ("stay", "move") and its divergent step always starts at the chain's
current point, so its cases ask for any divergence ("div")."""
import os

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import selftest_cases as SC
from helpers import assert_bit_exact, assert_vectors_bit_exact, estimator_pair, oracle_settings, sampling_launches
from test_gpu_host_callback_instantiations import coupled

pytestmark = pytest.mark.gpu

VECTORS = tuple(N.VECTOR_STATS)
EVENT_DIV = ("divergence_start", "divergence_start_gradient", "divergence_end")
EVENT_MM = ("mass_matrix_inv", "transformation_mu")
ALWAYS = ("gradient", "transformed_position", "transformed_gradient")
LOCKSTEP_VECTORS = ALWAYS                       # what nuts_lockstep.hpp writes besides positions and statistics
KINDS = {"nuts": 0, "exact": 1, "micro": 2}
LOW = 0.25                                      # max_energy_error of the cases that force divergences
WALL = 1.25                                     # host callback: a recoverable error beyond it (keyed on the last coordinate)

CONDITIONS = {
    "div0": "a divergent draw whose divergent leapfrog started at the trajectory's initial point (divergence_start == the previous position)",
    "divN": "a divergent draw whose divergent leapfrog started elsewhere",
    "div": "a divergent draw",
    "mm": "a mass-matrix event after draw 0",
    "stay": "a draw that stays on its initial point",
    "move": "a draw that moves",
    "tune": "draws on both sides of the end of tuning",
    "eig": "a mass-matrix event whose transformation has a low-rank part (a mass_matrix_eigvals row)",
    "wall": "a divergent draw caused by a recoverable error: no energy error, no end point",
}
NUTS_CONDS = ("div0", "divN", "mm", "stay", "move", "tune")
MCLMC_CONDS = ("div", "mm", "tune")


def _case(fam, name, seed, kind="nuts", dens="diag", dim=0, chains=3, tune=35, draws=65, cut=33, tiling=None, engine=None, skw=None,
          conds=None, lr=None, rank=0, order=0, vectors=None, served="wave", env=None):
    """One case.  tiling: (doubles per lane, wavefronts per chain) forced on the engine and asserted; served: the launches the case asserts
    ("wave", "group", "lane", "tile", "lockstep", "cluster"); lr: None | "adapt" | "shared" | "per_chain" | "hostcb"; order: the oracle's
    lr_seq_dots; vectors: what the case asks for (None: everything the settings store)."""
    conds = tuple(conds if conds is not None else (MCLMC_CONDS if kind == "mclmc" else NUTS_CONDS))
    return dict(fam=fam, id=f"{fam}-{name}", seed=seed, kind=kind, dens=dens, dim=dim, chains=chains, tune=tune, draws=draws, cut=cut,
                tiling=tiling, engine=dict(engine or {}), skw=dict(skw or {}), conds=conds, lr=lr, rank=rank, order=order, vectors=vectors,
                served=served, env=dict(env or {}))


ONE_CHAIN = dict(lane_groups=1, lane_chains=1, chain_tiles=1)        # the one-chain-per-block kernels, nothing else


def tiling_dims():
    """(tiling) -> (ragged odd dim, full tile), from the iid rows of the package's own list: the first dim the tiling serves by itself (one past
    the previous capacity; the (2,1) tiling has no previous one and takes its ragged top row, 125) and its capacity."""
    out = {}
    rows = [c for c in SC.cases() if c["dens"] == "iid" and c["fam"] == "nuts"]
    for (d, w) in SC.TILINGS:
        dims = sorted(c["dim"] for c in rows if (c["dpl"], c["w"]) == (d, w))
        ragged = [x for x in dims if x % 2 == 1 and x < d * 64 * w]
        out[(d, w)] = (ragged[0], d * 64 * w)
    return out


# ---- the case lists: the seeds are tools/small_chain_dry_run.py --only vectors' ----------------------------------------------------------------
SEEDS = {"C-mclmc-16x1-dim1021-ladder": 16, "D-mclmc-diag-dim4097-ladder": 2}


def family_a():
    out = []
    for (d, w), (ragged, full) in tiling_dims().items():
        for dim in (ragged, full):
            out.append(_case("A", f"diag-{d}x{w}-dim{dim}", 0, dim=dim, tiling=(d, w), engine=ONE_CHAIN, skw=dict(max_energy_error=LOW)))
    out.append(_case("A", "funnel-2x1-dim31", 0, dens="funnel", dim=31, chains=6, tune=40, draws=70, tiling=(2, 1), engine=ONE_CHAIN))
    out.append(_case("A", "funnel-4x1-dim131", 0, dens="funnel", dim=131, chains=6, tune=40, draws=70, tiling=(4, 1), engine=ONE_CHAIN))
    # the full-precision normal keeps its position vector in LDS, and emit_divergence_vectors' re-evaluation uses it again
    out.append(_case("A", "mvn-4x1-dim131", 0, dens="mvn", dim=131, tiling=(4, 1), engine=ONE_CHAIN, skw=dict(max_energy_error=LOW)))
    return out


def family_b():
    out = [
        # (the full-precision normal: a correlated target, so that the estimator finds eigenvalues and mass_matrix_eigvals rows are written)
        _case("B", "adapt-2x1-dim12", 0, dens="mvn", dim=12, chains=4, tune=60, draws=81, cut=41, lr="adapt", tiling=(2, 1), engine=ONE_CHAIN,
              skw=dict(max_energy_error=LOW), conds=NUTS_CONDS + ("eig",)),
        _case("B", "adapt-8x2-dim300", 0, dens="mvn", dim=300, chains=3, tune=60, draws=81, cut=41, lr="adapt", tiling=(8, 2), engine=ONE_CHAIN,
              skw=dict(max_energy_error=LOW, maxdepth=5), conds=NUTS_CONDS + ("eig",)),
        _case("B", "per_chain-2x1-dim70-rank3", 0, dim=70, lr="per_chain", rank=3, tiling=(2, 1), engine=ONE_CHAIN,
              skw=dict(max_energy_error=LOW), conds=("div0", "divN", "stay", "move", "tune")),
    ]
    for dim, rank, chains in ((64, 16, 21), (200, 200, 16)):
        shape = f"dim{dim}-rank{rank}"
        common = dict(dens="mvn", dim=dim, chains=chains, lr="shared", rank=rank, tiling=(4, 1), skw=dict(max_energy_error=LOW, maxdepth=6))       # (16 to 21 chains: trees to depth 6 keep the oracle's side to a second or two)
        out.append(_case("B", f"tile-{shape}", 0, engine=dict(chain_tiles=2), order=1, served="tile",
                         conds=("div0", "divN", "stay", "move", "tune"), **common))
        out.append(_case("B", f"auto_tile-{shape}", 0, engine=dict(chain_tiles=0), order=1, served="tile",
                         conds=("div0", "divN", "stay", "move", "tune"), **common))
        # "stay" and "move": nuts_lockstep.hpp stores the draw's x / g_x rows at two sites — a draw that stays on the stored point copies them
        # from the persistent slots in P3 (M_KEEP), a draw that moves writes them from the recomputing product (M_RECOMP); both cases reach both
        out.append(_case("B", f"lockstep-{shape}", 0, engine=dict(chain_tiles=3), order=2, served="lockstep", vectors=LOCKSTEP_VECTORS,
                         conds=("stay", "move", "tune"), **common))
    return out


def family_c():
    out = []
    for kind in ("exact", "micro", "mclmc"):
        for (d, w), dim in (((16, 1), 1021), ((4, 4), 1024)):
            skw, dens = dict(max_energy_error=LOW), "diag"
            if kind == "mclmc":
                # (16,1): dynamic_step_size with a step at which the halving ladder runs (average_step_size below the base step is asserted);
                # (4,4): a static step on the iid normal (on the diagonal normal a static step from U(-1, 1) diverges in every draw or in none)
                skw = (dict(step_size=1.5, max_energy_error=3.0, dynamic_step_size=True) if w == 1 else
                       dict(step_size=0.3, max_energy_error=2.0, dynamic_step_size=False))
                dens = "diag" if w == 1 else "iid"
            out.append(_case("C", f"{kind}-{d}x{w}-dim{dim}" + ("-ladder" if kind == "mclmc" and w == 1 else ""), 0, kind=kind, dens=dens, dim=dim,
                             tiling=(d, w), engine=ONE_CHAIN, skw=skw))
    return out


def family_d():
    out = []
    for dim in (4097, 8193):
        for dens in ("iid", "diag"):
            out.append(_case("D", f"nuts-{dens}-dim{dim}", 0, dens=dens, dim=dim, chains=2, tiling=(16, 4), served="cluster",
                             skw=dict(max_energy_error=LOW)))
    out.append(_case("D", "exact-diag-dim4097", 0, kind="exact", dim=4097, chains=2, tiling=(16, 4), served="cluster", skw=dict(max_energy_error=LOW)))
    out.append(_case("D", "micro-diag-dim4097", 0, kind="micro", dim=4097, chains=2, tiling=(16, 4), served="cluster", skw=dict(max_energy_error=LOW)))
    out.append(_case("D", "mclmc-diag-dim4097-ladder", 0, kind="mclmc", dim=4097, chains=2, tiling=(16, 4), served="cluster",
                     skw=dict(step_size=1.5, max_energy_error=3.0, dynamic_step_size=True)))
    out.append(_case("D", "nuts-diag-dim8193-general_exchange", 0, dim=8193, chains=2, tiling=(16, 4), served="cluster",
                     skw=dict(max_energy_error=LOW), env=dict(NM_CLUSTER_GENERAL="1")))
    return out


HOSTCB = dict(dens="hostcb", tune=20, draws=37, cut=19)      # the callback is Python on both sides: shorter runs, trees to depth 5


def family_e():
    skw = dict(max_energy_error=LOW, maxdepth=5)
    out = [
        _case("E", "hostcb-2x1-dim125", 0, dim=125, tiling=(2, 1), engine=ONE_CHAIN, skw=skw, **HOSTCB),
        _case("E", "hostcb-4x4-dim1024", 0, dim=1024, tiling=(4, 4), engine=ONE_CHAIN, skw=skw, **HOSTCB),
        _case("E", "hostcb-16x4-dim4093", 0, dim=4093, tiling=(16, 4), engine=ONE_CHAIN, skw=skw, **HOSTCB),
        _case("E", "lr_hostcb-2x1-dim70", 0, dim=70, lr="hostcb", rank=3, tiling=(2, 1), engine=ONE_CHAIN, skw=skw,
              conds=("div0", "divN", "stay", "move", "tune"), **HOSTCB),
        _case("E", "micro_hostcb-2x1-dim70", 0, kind="micro", dim=70, tiling=(2, 1), engine=ONE_CHAIN, skw=skw, **HOSTCB),
        _case("E", "hostcb-wide-dim4500", 0, dim=4500, chains=2, tiling=(16, 4), served="cluster", skw=skw, **HOSTCB),
        # the reference's recoverable error (src/dynamics/transformed_hamiltonian.rs:562-578): a divergence without an end point
        _case("E", "wall-2x1-dim125", 0, dim=125, tiling=(2, 1), engine=ONE_CHAIN, skw=dict(maxdepth=5), conds=("wall", "mm", "stay", "move", "tune"),
              **dict(HOSTCB, dens="hostcb_wall")),
        _case("E", "wall-16x4-dim4093", 0, dim=4093, tiling=(16, 4), engine=ONE_CHAIN, skw=dict(maxdepth=5), conds=("wall", "mm", "stay", "move", "tune"),
              **dict(HOSTCB, dens="hostcb_wall")),
    ]
    return out


def family_f():
    grp = dict(lane_groups=2)
    return [
        # 8 / 4 / 2 chains per wavefront, the last wavefront partly filled
        _case("F", "group-exact-dim11", 0, kind="exact", dim=11, chains=21, tiling=(2, 1), engine=grp, served="group", skw=dict(max_energy_error=LOW)),
        _case("F", "group-micro-dim30", 0, kind="micro", dim=30, chains=9, tiling=(2, 1), engine=grp, served="group", skw=dict(max_energy_error=LOW)),
        _case("F", "group-mclmc-dim50", 0, kind="mclmc", dim=50, chains=5, tiling=(2, 1), engine=grp, served="group",
              skw=dict(step_size=0.1, max_energy_error=10.0, dynamic_step_size=False)),
        _case("F", "lane-exact-dim10", 0, kind="exact", dim=10, chains=70, tiling=(2, 1), engine=dict(lane_chains=2), served="lane",
              skw=dict(max_energy_error=LOW)),
        _case("F", "lane-micro-dim3", 0, kind="micro", dim=3, chains=70, tiling=(2, 1), engine=dict(lane_chains=2), served="lane",
              skw=dict(max_energy_error=LOW)),
    ]


def family_g():
    """The two cases whose vectors are requested one at a time and through the device path: A's ragged (2,1) case and A's ragged (16,1) case
    with the cut moved behind the end of tuning, so that the second launch is the sampling build's."""
    a = {c["id"]: c for c in family_a()}
    g1 = dict(a["A-diag-2x1-dim125"], fam="G", id="G-diag-2x1-dim125")
    g2 = dict(a["A-diag-16x1-dim513"], fam="G", id="G-diag-16x1-dim513-sampling", cut=39)
    return [g1, g2]


def all_cases():
    out = family_a() + family_b() + family_c() + family_d() + family_e() + family_f() + family_g()
    for c in out:
        c["seed"] = SEEDS.get(c["id"], c["seed"])
    return out


def by_family(fam):
    return [pytest.param(c, id=c["id"]) for c in all_cases() if c["fam"] == fam]


# ---- inputs, from exact operations only ----------------------------------------------------------------------------------------------------------
def index_precisions(dim):
    """precisions (1 + (i mod 8) / 8) * 2^((i mod 5) - 2): they depend on the coordinate's index, so a row stored at a wrong element shows"""
    i = np.arange(dim)
    return np.ldexp(1.0 + (i % 8) / 8.0, (i % 5) - 2)


def exact_transform(dim, rank, seed, per_chain=0):
    """(stds, mean, eigenvalues, orthonormal eigenvectors [rank][dim], gradient mean) of exactly representable numbers: the eigenvectors are
    rows of 4 x 4 Hadamard blocks over two (+-1/2 on four coordinates, rank <= dim - dim mod 4), with random signs."""
    if per_chain:
        parts = [exact_transform(dim, rank, seed + 101 * k) for k in range(per_chain)]
        return tuple(np.ascontiguousarray(np.stack([p[j] for p in parts])) for j in range(5))
    r = np.random.default_rng(seed)
    h = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=np.float64) / 2.0
    assert rank <= dim - dim % 4
    vecs = np.zeros((rank, dim))
    for k in range(rank):
        vecs[k, 4 * (k // 4):4 * (k // 4) + 4] = h[k % 4] * (1 - 2 * int(r.integers(0, 2)))
    return (SC._dyadic(r, dim, -1, 1), r.integers(-16, 17, dim) / 16.0, SC._dyadic(r, rank, -1, 2), np.ascontiguousarray(vecs),
            r.integers(-8, 9, dim) / 16.0)


def make_transform(c):
    if c["lr"] in ("shared", "hostcb"):
        return exact_transform(c["dim"], c["rank"], 7 + c["dim"])
    if c["lr"] == "per_chain":
        return exact_transform(c["dim"], c["rank"], 7 + c["dim"], per_chain=c["chains"])
    return None


def wall_density(dim):
    last = dim - 1

    def density(chain, x):
        if x[last] > WALL:
            raise N.RecoverableLogpError("outside the support")
        return coupled(chain, x)
    return density


def host_density(c):
    return wall_density(c["dim"]) if c["dens"] == "hostcb_wall" else coupled


def make_logp(c, host_fn=None):
    dens, dim = c["dens"], c["dim"]
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    if dens == "diag":
        return N.LogpSpec.diag_normal(index_precisions(dim))
    if dens == "funnel":
        return N.LogpSpec.funnel(dim)
    if dens == "mvn":
        return SC.make_logp(N, "mvn", dim, 1)
    return N.LogpSpec.host_callback(dim, host_fn or host_density(c), threads=2)


def make_settings(c):
    """every store_* switch on (for the low-rank settings that includes store_mass_matrix, hence mass_matrix_eigvals)"""
    kw = dict(num_chains=c["chains"], seed=c["seed"], num_tune=c["tune"], store_gradient=True, store_unconstrained=True, store_transformed=True,
              store_divergences=True, **c["skw"])
    if c["kind"] == "mclmc":
        s = N.DiagMclmcSettings(**kw)
        s.adapt_options.mass_matrix_options.store_mass_matrix = True
    elif c["lr"]:
        s = N.LowRankNutsSettings(store_mass_matrix=True, freeze_transform=c["lr"] != "adapt", **kw)
        if c["lr"] == "adapt":
            s.adapt_options.mass_matrix_update_freq = 5
    else:
        s = N.DiagNutsSettings(trajectory_kind=KINDS[c["kind"]], **kw)
        s.adapt_options.mass_matrix_options.store_mass_matrix = True
    return s


def threads_per_chain(c):
    return 64 * c["tiling"][1]


def oracle_cfg(O, c):
    return O.gpu_cfg(threads_per_chain(c), lr_seq_dots=c["order"], gpu_slice=4096 if c["served"] == "cluster" else 0)


# ---- the oracle's side (CPU only: the dry run calls it too) ------------------------------------------------------------------------------------
def oracle_side(O, c, estimator=None):
    """-> dict(x0, pos, st, vec [all nine], calls [host callback: evaluations of the density])"""
    s = make_settings(c)
    so, cfg, n, dim, draws = oracle_settings(O, s), oracle_cfg(O, c), c["chains"], c["dim"], c["draws"]
    x0 = O.init_positions_uniform(s.seed, 0, n, dim)
    transform = make_transform(c)
    if not c["dens"].startswith("hostcb"):
        logp = make_logp(c)
        vec = {}
        if c["lr"] == "adapt" and estimator is None:
            estimator = estimator_pair(O)[0]
        pos, st, _, failed = O.run(so, logp.kind, dim, logp.params, cfg, n, x0, draws, n_threads=min(n, 8), vectors=vec, transform=transform,
                                   estimator=estimator)
        return dict(x0=x0, pos=pos, st=st, vec=vec, failed=list(range(failed)), calls=0)
    fn, calls = host_density(c), [0]

    def tramp(ctx, d, px, pg, plogp):
        calls[0] += 1
        try:
            lp, g = fn(0, np.ctypeslib.as_array(px, shape=(d,)).copy())
        except N.RecoverableLogpError:
            return 1
        np.ctypeslib.as_array(pg, shape=(d,))[:] = g
        plogp[0] = lp
        return 0
    cb = O.HOST_LOGP_FN(tramp)
    pos = np.full((draws, n, dim), np.nan)
    st = np.zeros((draws, n), dtype=O.STATS_DTYPE)
    vec = {k: np.full((draws, n, dim), np.nan) for k in O.VECTOR_STATS}
    failed = []
    for k in range(n):
        ch = O.Chain(so, 0, dim, np.zeros(1), cfg, chain_id=k, callback=cb)
        if ch.set_position(x0[k]) != 0:
            failed.append(k)
            continue
        if transform is not None:
            assert ch.set_transform(*transform) == 1
        for t in range(draws):
            row = {}
            pos[t, k], st[t, k], rc = ch.draw(vectors=row)
            if rc != 0:
                failed.append(k)
                break
            for name in vec:
                vec[name][t, k] = row[name]
    return dict(x0=x0, pos=pos, st=st, vec=vec, failed=failed, calls=calls[0])


def bits_equal(a, b):
    return (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64))


def events(c, x0, pos, st, vec):
    """What happened in a run, from its statistics and its divergence_start rows."""
    div = st["diverging"] != 0
    prev = np.concatenate([x0[None], pos[:-1]])
    out = dict(div=div, upd=st["transformation_update_id"] >= 0, stay=st["index_in_trajectory"] == 0,
               wall=div & np.isnan(st["divergence_energy_error"]))
    if "divergence_start" in vec:
        at_start = bits_equal(vec["divergence_start"], prev).all(axis=2)
        out.update(div0=div & at_start, divN=div & ~at_start)
    return out


def findings(c, x0, pos, st, vec):
    """The case's conditions that the run does not meet: -> a list of complaints (empty: fine)."""
    e = events(c, x0, pos, st, vec)
    have = dict(div=e["div"].any(), mm=e["upd"][1:].any(), stay=e["stay"].any(), move=(~e["stay"]).any(),
                tune=bool((st["tuning"] != 0).any() and (st["tuning"] == 0).any()), wall=e["wall"].any(), eig=(st["num_eigenvalues"] > 0).any(),
                div0=e.get("div0", np.zeros(1, dtype=bool)).any(), divN=e.get("divN", np.zeros(1, dtype=bool)).any())
    out = [f"no {CONDITIONS[k]}" for k in c["conds"] if not have[k]]
    if "wall" in c["conds"] and "divergence_end" in vec and e["wall"].any():
        if not np.isnan(vec["divergence_end"][e["wall"]]).all() or np.isnan(vec["divergence_start"][e["wall"]]).any():
            out.append("a recoverable error's divergence has an end point or no start point")
    if not (st["chain_status"] == 0).all() or not np.isfinite(pos).all():
        out.append("a chain failed")
    if "-ladder" in c["id"] and not (st["average_step_size"] < c["skw"]["step_size"] * (1 - 1e-12)).any():
        out.append("the step-halving ladder never ran")
    return out


_ORACLE = {}


def oracle_cached(O, c, estimator=None):
    """the reference of a case, computed once and shared (G's tests read the same one several times); never modified"""
    if c["id"] not in _ORACLE or estimator is not None:
        _ORACLE[c["id"]] = oracle_side(O, c, estimator)
    return _ORACLE[c["id"]]


# ---- the engine's side --------------------------------------------------------------------------------------------------------------------------
def engine_kwargs(c):
    """the engine's configuration: the case's own switches, and its tiling forced where the family lets a caller choose one (a wide chain has
    one tiling; the matrix-core kernels take the 4-doubles tiling only when the choice is left to the engine: engine_plan.hpp auto_dpl)"""
    d, w = c["tiling"]
    kw = dict(c["engine"])
    if c["served"] not in ("cluster", "tile", "lockstep"):
        kw.update(dims_per_lane=d, waves_per_chain=w)
    return kw


def open_engine(O, c, host_fn=None, estimator=None):
    s = make_settings(c)
    b = N.ChainBatch(s, make_logp(c, host_fn), c["chains"], **engine_kwargs(c))
    try:
        x0 = O.init_positions_uniform(s.seed, 0, c["chains"], c["dim"])
        assert (b.set_position(x0, raise_on_error=False) == 0).all()
        if estimator is not None:
            b.set_lowrank_estimator(estimator, n_threads=1)
        transform = make_transform(c)
        if transform is not None:
            b.set_transform(*transform)
    except BaseException:
        b.close()
        raise
    return b, x0


def assert_served(b, c, launches=2):
    """which kernel served the case, from the engine's counters and accessors"""
    d, w = c["tiling"]
    served = c["served"]
    assert (b.dims_per_lane(), b.threads_per_chain()) == (d, 64 * w)
    assert b.blocks_per_chain() == (-(-c["dim"] // 4096) if served == "cluster" else 1)
    # (a call that crosses the end of the warm-up may be cut into two launches: at least one launch per call)
    assert b.group_launches() >= launches if served == "group" else b.group_launches() == 0
    assert b.lane_launches() >= launches if served == "lane" else b.lane_launches() == 0
    assert b.tile_launches() >= launches if served in ("tile", "lockstep") else b.tile_launches() == 0
    assert b.lockstep_launches() == b.tile_launches() if served == "lockstep" else b.lockstep_launches() == 0
    assert b.reduce_order() == c["order"] == {"tile": 1, "lockstep": 2}.get(served, 0)
    # the sampling-phase build serves the draws after the warm-up of the plain family on its tilings (nuts_contract.hpp sampling_tiling)
    sampling = (served == "wave" and c["kind"] == "nuts" and not c["lr"] and w == 1 and d in (8, 16) and not c["dens"].startswith("hostcb") and
                c["draws"] > c["tune"] + 1)
    assert (sampling_launches(b) > 0) == sampling
    return sampling


def engine_side(O, c, vectors=None, host_fn=None, estimator=None):
    """two launches cut at c["cut"], concatenated -> dict(x0, pos, st, vec, host_calls, sampling)"""
    env = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        b, x0 = open_engine(O, c, host_fn, estimator)
        try:
            names = list(vectors if vectors is not None else c["vectors"] if c["vectors"] is not None else b.stored_vectors())
            if vectors is None and c["vectors"] is None:
                assert sorted(names) == sorted(k for k in VECTORS if k != "mass_matrix_eigvals" or c["lr"])
            cut = c["cut"]
            assert cut % 2 == 1 and 0 < cut < c["draws"]
            pa, sa, va = b.expanded_draw_many(cut, vectors=names)
            before = sampling_launches(b)
            pb, sb, vb = b.expanded_draw_many(c["draws"] - cut, vectors=names)
            sampling = assert_served(b, c)
            out = dict(x0=x0, pos=np.concatenate([pa, pb]), st=np.concatenate([sa, sb]), vec={k: np.concatenate([va[k], vb[k]]) for k in names},
                       host_calls=b.host_logp_calls(), sampling=sampling, sampling_second=sampling_launches(b) - before,
                       leapfrogs=b.counters()["total_leapfrogs"])
        finally:
            b.close()
    finally:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def assert_event_rows(c, st, vec):
    """exactly the event rows are written (the others keep the NaN the host arrays were given), the per-draw rows everywhere"""
    div, upd = st["diverging"] != 0, st["transformation_update_id"] >= 0
    for k in ALWAYS:
        if k in vec:
            assert np.isfinite(vec[k]).all(), k
    for k in ("divergence_start", "divergence_start_gradient"):
        if k in vec:
            assert (np.isnan(vec[k]).all(axis=2) == ~div).all() and not np.isnan(vec[k][div]).any(), k
    if "divergence_end" in vec:
        has_end = div & ~((st["diverging"] != 0) & np.isnan(st["divergence_energy_error"])) if "wall" in c["conds"] else div
        assert (np.isnan(vec["divergence_end"]).all(axis=2) == ~has_end).all() and not np.isnan(vec["divergence_end"][has_end]).any()
    for k in EVENT_MM:
        if k in vec:
            assert (np.isnan(vec[k]).all(axis=2) == ~upd).all() and not np.isnan(vec[k][upd]).any(), k
    if "mass_matrix_eigvals" in vec:
        assert np.isnan(vec["mass_matrix_eigvals"][~upd]).all()
        assert upd[0].all()                                   # the first extraction compares with -1


def run_case(O, c):
    """Engine against oracle: positions, statistics, every vector, the event rows, the case's conditions.  -> (engine, oracle)"""
    cb_o = cb_e = None
    if c["lr"] == "adapt":
        cb_o, cb_e, rec = estimator_pair(O)
    calls = []                                   # (list.append is atomic: the engine calls from two service threads)
    host_fn = None
    if c["dens"].startswith("hostcb"):
        inner = host_density(c)

        def host_fn(chain, x):
            calls.append(chain)
            return inner(chain, x)
    g = engine_side(O, c, host_fn=host_fn, estimator=cb_e)
    o = oracle_cached(O, c, cb_o)
    assert not o["failed"], "an oracle chain failed: pick another seed (tools/small_chain_dry_run.py --only vectors)"
    assert_bit_exact(g["pos"], g["st"], o["pos"], o["st"])
    if c["kind"] == "mclmc":
        for f in ("energy_change", "average_step_size"):
            assert ((g["st"][f] == o["st"][f]) | (np.isnan(g["st"][f]) & np.isnan(o["st"][f]))).all(), f
    assert (g["st"]["num_eigenvalues"] == o["st"]["num_eigenvalues"]).all()
    assert_vectors_bit_exact(g["vec"], o["vec"])
    assert_event_rows(c, g["st"], g["vec"])
    assert findings(c, g["x0"], g["pos"], g["st"], g["vec"]) == [], "pick another seed (tools/small_chain_dry_run.py --only vectors)"
    if c["dens"].startswith("hostcb"):
        # Evaluations of the host density.  The oracle keeps x and g_x of every point of the tree; the engine keeps z and rebuilds: one more
        # evaluation for every draw that moves (chain_draw: the winner's x and g_x from its z; with the divergence vectors requested x / g_x
        # are stored after every draw, so a draw that stays re-evaluates nothing), and one for every divergent draw whose divergent leapfrog
        # did not start at the initial point (emit_divergence_vectors rebuilds the start point; the end point needs no gradient).
        e = events(c, g["x0"], g["pos"], g["st"], g["vec"])
        assert g["host_calls"] == len(calls)
        assert g["host_calls"] == o["calls"] + int((~e["stay"]).sum()) + int(e["divN"].sum()), (g["host_calls"], o["calls"], int((~e["stay"]).sum()), int(e["divN"].sum()))
    return g, o


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", by_family("A"))
def test_one_chain_kernels_every_tiling(oracle, case):
    """A: `write_row`'s masked-store loop at a ragged dim and at the full tile of each of the eight tilings; both arms of emit_divergence_vectors."""
    run_case(oracle, case)


@pytest.mark.parametrize("case", by_family("B"))
def test_low_rank_transformation(oracle, case):
    """B: LrWrap (emit_divergence_vectors rebuilds x through transform_to_x), the tile kernel and the lockstep kernel.  The lockstep cases ask
    for gradient, transformed_position and transformed_gradient — all it writes; what it refuses: test_lockstep_refuses_event_vectors."""
    g, _ = run_case(oracle, case)
    if case["served"] == "lockstep":
        assert sorted(g["vec"]) == sorted(LOCKSTEP_VECTORS)
    if "eig" in case["conds"]:
        has = g["st"]["num_eigenvalues"] > 0
        assert not np.isnan(g["vec"]["mass_matrix_eigvals"][has][:, 0]).any() and np.isnan(g["vec"]["mass_matrix_eigvals"][~has]).all()


@pytest.mark.parametrize("chain_tiles", [0, 3])
def test_lockstep_refuses_event_vectors(oracle, chain_tiles):
    """REFUSED: a divergence or mass-matrix vector from the lockstep kernel — NM_ERR_UNSUPPORTED with `lockstep_outputs_error`'s text
    (csrc/engine_plan.hpp), for the engine that chose the kernel by itself (settings without store_divergences / store_mass_matrix) and for
    the one that was told to (chain_tiles = 3).  Nothing is launched, and the vectors the kernel does write are still served afterwards."""
    c = dict([x for x in family_b() if x["id"] == "B-lockstep-dim64-rank16"][0])
    s = make_settings(c)
    if chain_tiles == 0:
        s.store_divergences = False
        s.adapt_options.mass_matrix_options.store_mass_matrix = False
    b = N.ChainBatch(s, make_logp(c), c["chains"], chain_tiles=chain_tiles)
    try:
        assert (b.set_position(oracle.init_positions_uniform(s.seed, 0, c["chains"], c["dim"])) == 0).all()
        b.set_transform(*make_transform(c))
        want = ("this engine chose the lockstep matrix-core kernel (settings without store_divergences / store_mass_matrix), which writes positions, "
                "statistics, gradient and the transformed point only; set store_divergences / store_mass_matrix in the settings (the engine then "
                "takes the tile kernel from the start: the two sum over dim in different orders) or chain_tiles = 2" if chain_tiles == 0 else
                "the lockstep matrix-core kernel writes positions, statistics, gradient and the transformed point only; "
                "create the engine with chain_tiles = 2 for the divergence / mass-matrix vectors")
        for name in EVENT_DIV + EVENT_MM + ("mass_matrix_eigvals",):
            before = b.counters()
            with pytest.raises(N.NutsAmdError) as e:
                b.expanded_draw_many(3, vectors=[name])
            assert e.value.status == 4 and str(e.value) == "NM_ERR_UNSUPPORTED: " + want, name
            assert b.counters()["total_draws"] == before["total_draws"]
        _, st, vec = b.expanded_draw_many(3, vectors=list(LOCKSTEP_VECTORS))
        assert b.lockstep_launches() == 1 and b.reduce_order() == 2 and (st["draw"][:, 0] == [0, 1, 2]).all()
        assert all(np.isfinite(vec[k]).all() for k in LOCKSTEP_VECTORS)
    finally:
        b.close()


@pytest.mark.parametrize("case", by_family("C"))
def test_trajectory_kinds_and_mclmc(oracle, case):
    """C: KinWrap's draw loops (ExactNormal, Microcanonical, MCLMC) on a one-wavefront and a four-wavefront tiling."""
    run_case(oracle, case)


@pytest.mark.parametrize("case", by_family("D"))
def test_wide_chains(oracle, case):
    """D: `write_row` adds the block's slice offset to every row: every element of every row is compared, so a dropped or doubled offset shows
    (dim 4097: the second block owns ONE element)."""
    run_case(oracle, case)


@pytest.mark.parametrize("case", by_family("E"))
def test_host_callback(oracle, case):
    """E: the host-callback kernels; emit_divergence_vectors' re-evaluation is one more mailbox round trip, and a recoverable error leaves the
    end row unwritten while the start rows are written."""
    g, _ = run_case(oracle, case)
    if "wall" in case["conds"]:
        assert (g["pos"][..., case["dim"] - 1] <= WALL).all()


@pytest.mark.parametrize("case", by_family("F"))
def test_group_and_lane_kernels_beyond_euclidean(oracle, case):
    """F: the several-chains-per-wavefront and one-chain-per-lane kernels' own `P.out_*` sites under the non-Euclidean kinds."""
    run_case(oracle, case)


@pytest.mark.parametrize("case", by_family("G"))
def test_one_vector_requested_alone(oracle, case):
    """G: every vector alone, from an identically seeded fresh engine: its rows and the positions equal the all-vectors run's (shown equal to
    the oracle's), bit for bit and NaN for NaN.  `want_div` includes out_div_end, `need_x` does not, and px_stale depends on both."""
    O = oracle
    full, o = run_case(O, case)
    if "sampling" in case["id"]:
        assert full["sampling_second"] >= 1
    names = [k for k in VECTORS if k != "mass_matrix_eigvals"]
    assert sorted(full["vec"]) == sorted(names)
    for name in names:
        g = engine_side(O, case, vectors=[name])
        try:
            assert_bit_exact(g["pos"], g["st"], full["pos"], full["st"])
            assert list(g["vec"]) == [name]
            assert_vectors_bit_exact(g["vec"], {name: full["vec"][name]})
            assert (np.isnan(g["vec"][name]) == np.isnan(full["vec"][name])).all()
        except AssertionError as e:
            raise AssertionError(f"{name} requested alone: {e}") from None


SENTINEL = np.array([0x4B1DC0DEC0FFEE11], dtype=np.uint64).view(np.float64)[0]      # a finite double no draw produces


@pytest.mark.parametrize("case", by_family("G"))
def test_device_path_leaves_other_rows_untouched(oracle, case):
    """G: `nm_engine_draw_ex` into device buffers pre-filled with a non-NaN bit pattern, in two launches, the second into the same buffers at
    the row offset: event rows are the oracle's, every other row still holds the pattern (include/nuts_amd.h: "other rows are left untouched")."""
    import torch
    O, c = oracle, case
    o = oracle_cached(O, c)
    n, dim, draws, cut = c["chains"], c["dim"], c["draws"], c["cut"]
    names = [k for k in VECTORS if k != "mass_matrix_eigvals"]
    bufs = {k: torch.full((draws, n, dim), float(SENTINEL), dtype=torch.float64, device="cuda") for k in names + ["positions"]}
    d_st = torch.zeros((draws, n, N.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b, x0 = open_engine(O, c)
    try:
        for lo, k in ((0, cut), (cut, draws - cut)):
            b.draw_device_ex(k, positions=bufs["positions"][lo:].data_ptr(), stats=d_st[lo:].data_ptr(),
                             **{name: bufs[name][lo:].data_ptr() for name in names})
        sampling = assert_served(b, c)
        assert sampling == ("sampling" in c["id"])
    finally:
        b.close()
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    st = d_st.cpu().numpy().reshape(-1).view(N.STATS_DTYPE).reshape(draws, n)
    assert_bit_exact(got["positions"], st, o["pos"], o["st"])
    div, upd = st["diverging"] != 0, st["transformation_update_id"] >= 0
    written = {k: np.ones((draws, n), dtype=bool) for k in ALWAYS}
    written.update({k: div for k in EVENT_DIV})
    written.update({k: upd for k in EVENT_MM})
    assert div.any() and not div.all() and upd.any() and not upd.all()
    for k in names:
        w = written[k]
        assert bits_equal(got[k][w], o["vec"][k][w]).all(), k
        assert not np.isnan(o["vec"][k][w]).any(), k
        assert bits_equal(got[k][~w], np.full_like(got[k][~w], SENTINEL)).all(), f"{k}: a row whose event did not happen was written"
