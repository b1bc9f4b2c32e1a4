"""The doubling boundary of the (16 doubles, 1 wavefront) kernels with register end points and gradient-free points (nuts_kernels.hpp
`reg_edges && nog_mode`: iid and diagonal normal): where a finished doubling's end point is written to the end-point registers, where the
next doubling reads the end it starts from, and the top-level U-turn tests that read all four tiles.  Bit for bit against the oracle:
positions and every statistics field, on the general build (the warm-up's launches) and on the sampling build.

The statistics rows do not say which way a doubling went, so the tree shapes are read off the oracle's random stream: the chain's word
position before and after a draw (oracle.Chain.state) brackets the draw's words, the momentum refresh is replayed on them (`refresh_end`:
the ziggurat of nmo_rng.hpp on the words of nmo_rng_words), and the direction words follow at offsets that depend only on how many of the
merges into the main tree drew a Bernoulli word (`directions`).  A draw counts for a shape only when every placement of those merges
that is consistent with the draw's word count gives the same directions; each case asserts on these rows first that its seeds hold the
shapes it is about, on both builds."""
import functools
import itertools

import numpy as np
import pytest

import nuts_rs_amd as N
from helpers import assert_bit_exact, oracle_settings, sampling_launches

pytestmark = pytest.mark.gpu

N_CHAINS, NUM_TUNE, N_POST = 3, 12, 30
N_DRAWS = NUM_TUNE + N_POST
N_GENERAL = NUM_TUNE + 1              # draws the general kernel serves: the warm-up and the draw that re-whitens after its last update
DIMS = [513, 1024]
DENS = ["iid", "diag"]
SEEDS = {("iid", 513): 701, ("iid", 1024): 705, ("diag", 513): 700, ("diag", 1024): 700}


def make_logp(dens, dim):
    if dens == "iid":
        return N.LogpSpec.iid_normal(dim, 3.0)
    return N.LogpSpec.diag_normal(np.exp(np.random.default_rng(dim).uniform(-2, 2, dim)))


def make_settings(dens, dim, **kw):
    return N.DiagNutsSettings(num_chains=N_CHAINS, seed=SEEDS[dens, dim], num_tune=NUM_TUNE, **kw)


# ---- the oracle's run, with the word position of every chain's random stream around every draw ----
@functools.lru_cache(maxsize=None)
def oracle_run(dens, dim, **kw):
    """one oracle run per configuration, shared by the cases that compare against it -> x0, positions, rows, word positions [draws + 1][chains]"""
    from oracle import oracle as O
    s, logp = make_settings(dens, dim, **kw), make_logp(dens, dim)
    x0 = O.init_positions_uniform(s.seed, 0, N_CHAINS, dim)
    pos = np.empty((N_DRAWS, N_CHAINS, dim))
    st = np.zeros((N_DRAWS, N_CHAINS), dtype=O.STATS_DTYPE)
    wp = np.zeros((N_DRAWS + 1, N_CHAINS), dtype=np.int64)
    for c in range(N_CHAINS):
        ch = O.Chain(oracle_settings(O, s), logp.kind, dim, logp.params, O.gpu_cfg(64), chain_id=c)
        assert ch.set_position(x0[c]) == 0
        wp[0, c] = ch.state()["rng_pos"]
        for t in range(N_DRAWS):
            pos[t, c], st[t, c], rc = ch.draw()
            assert rc == 0
            wp[t + 1, c] = ch.state()["rng_pos"]
    for a in (pos, st, wp):
        a.setflags(write=False)
    return x0, pos, st, wp


@functools.lru_cache(maxsize=None)
def chain_words(seed, chain, count):
    """words 0 .. count-1 of the chain's ChaCha8 stream as Python ints"""
    from oracle import oracle as O
    out = np.empty(count, dtype=np.uint32)
    O.lib().nmo_rng_words(O.chain_key(seed, chain), 0, count, out.ctypes.data)
    return [int(w) for w in out]


@functools.lru_cache(maxsize=None)
def zig_tables():
    from oracle import oracle as O
    x, f = np.empty(257), np.empty(257)
    O.lib().nmo_zig_tables(x, f)
    return x.tolist(), f.tolist()


def refresh_end(words, p, dim):
    """word position after `dim` standard normals drawn from position p: rand_distr's ziggurat as nmo_rng.hpp restates it"""
    import ctypes as C
    from oracle import oracle as O
    X, F = zig_tables()
    cfg = O.gpu_cfg(64)
    fn = lambda op, a: O.lib().nmo_scalar_fn(C.byref(cfg), op, a, 0.0)
    u64 = lambda q: words[q] | (words[q + 1] << 32)
    as_f64 = lambda bits: float(np.uint64(bits).view(np.float64))
    R = X[1]                                                     # ZIG_NORM_R: the start of the tail
    for _ in range(dim):
        while True:
            bits = u64(p); p += 2
            i = bits & 0xff
            u = as_f64((bits >> 12) | 0x4000000000000000) - 3.0
            x = u * X[i]
            if abs(x) < X[i + 1]:
                break
            if i == 0:
                xx, yy = 1.0, 0.0
                while -2.0 * yy < xx * xx:
                    a = as_f64((u64(p) >> 12) | 0x3ff0000000000000) - (1.0 - 2.220446049250313e-16 / 2.0); p += 2
                    b = as_f64((u64(p) >> 12) | 0x3ff0000000000000) - (1.0 - 2.220446049250313e-16 / 2.0); p += 2
                    xx, yy = fn(1, a) / R, fn(1, b)
                break
            f64 = float(u64(p) >> 11) * (1.0 / 9007199254740992.0); p += 2
            if F[i + 1] + (F[i] - F[i + 1]) * f64 < fn(0, -x * x / 2.0):
                break
    return p


def directions(words, p0, p1, dim, depth, jitter_words=2):
    """The directions (+1 / -1 per doubling) of a draw whose tree has `depth` complete doublings and no discarded one, from the words
    p0 .. p1 of its chain's stream, or None when the words do not pin them.  After the refresh, doubling j costs one direction word, two
    words for each of its 2^j - 1 merges inside `other`, and two more when its merge into the main tree drew a Bernoulli word (m_j = 1);
    the step-size jitter takes the draw's last two words."""
    q0 = refresh_end(words, p0, dim)
    fixed = sum(1 + 2 * ((1 << j) - 1) for j in range(depth))
    spare = p1 - jitter_words - q0 - fixed
    if spare < 0 or spare % 2 or spare // 2 > depth:
        return None                                              # (a draw followed by a step-size search, a merge with p = 1, ...)
    found = set()
    for m in itertools.product((0, 1), repeat=depth):
        if sum(m) != spare // 2:
            continue
        q, dirs = q0, []
        for j in range(depth):
            dirs.append(1 if words[q] >> 31 else -1)
            q += 1 + 2 * ((1 << j) - 1) + 2 * m[j]
        found.add(tuple(dirs))
    return found.pop() if len(found) == 1 else None


def tree_shapes(dens, dim, st, wp, maxdepth):
    """per build ('general' / 'sampling'): the set of shapes its draws show.  'turn@k': the tree changed direction at doubling k (k = 1, 2,
    3); 'straight': a tree of >= 2 doublings that never changed it; 'initial': the draw is the trajectory's initial point after >= 1
    doubling; 'top_uturn': the tree ended on a U-turn of the top-level tests (every doubling complete, below maxdepth, no divergence)."""
    seed = SEEDS[dens, dim]
    shapes = {"general": set(), "sampling": set()}
    for c in range(N_CHAINS):
        words = chain_words(seed, c, int(wp[-1, c]) + 64)
        for t in range(N_DRAWS):
            r, build = st[t, c], "general" if t < N_GENERAL else "sampling"
            d = int(r["depth"])
            if r["diverging"] or int(r["n_steps"]) != (1 << d) - 1:
                continue                                         # a discarded doubling: the word count says nothing simple
            if d >= 1 and int(r["index_in_trajectory"]) == 0:
                shapes[build].add("initial")
            if d < maxdepth and d >= 1:
                shapes[build].add("top_uturn")
            # (a merge inside `other` draws no word when its probability rounds to 1: leaf weights 2^53 apart.  Energy errors below 10
            # keep the log-sizes of two sub-trees of <= 2^7 leaves within 2 * 10 + 7 ln 2 < 53 ln 2 of each other.)
            calm = abs(float(r["max_energy_error"])) < 10.0
            dirs = directions(words, int(wp[t, c]), int(wp[t + 1, c]), dim, d) if 1 <= d <= 8 and calm else None
            if dirs is None:
                continue
            lo, hi = -sum(1 << j for j in range(d) if dirs[j] < 0), sum(1 << j for j in range(d) if dirs[j] > 0)
            assert lo <= int(r["index_in_trajectory"]) <= hi, (dens, dim, t, c, dirs)       # the replay agrees with the row
            for k in range(1, min(d, 4)):
                if dirs[k] != dirs[k - 1]:
                    shapes[build].add(f"turn@{k}")
            if d >= 2 and len(set(dirs)) == 1:
                shapes[build].add("straight")
    return shapes


def engine_run(dens, dim, counts=(N_DRAWS,), **kw):
    """the run on the engine, one draw_many per entry of `counts` -> positions, statistics, launches of the sampling build per call"""
    x0 = oracle_run(dens, dim, **kw)[0]
    b = N.ChainBatch(make_settings(dens, dim, **kw), make_logp(dens, dim), N_CHAINS)
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


def check_case(dens, dim, **kw):
    _, pos_o, st_o, _ = oracle_run(dens, dim, **kw)
    pos_g, st_g, served = engine_run(dens, dim, (N_GENERAL, N_DRAWS - N_GENERAL), **kw)
    assert served == [0, 1], "the warm-up on the general kernel, the rest in one launch of the sampling build"
    assert_bit_exact(pos_g, st_g, pos_o, st_o)


ALL_SHAPES = {"turn@1", "turn@2", "turn@3", "straight", "initial", "top_uturn"}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_every_tree_shape_on_both_builds(oracle, dens, dim):
    """maxdepth 10: trees that change direction at doubling 1, 2 and 3 and a U-turn at the top level on the general and on the sampling build,
    and a re-whitening draw in the warm-up.  With the depth-limited runs of this density and dim (test_depth_limit, the same seed) each build
    also sees trees that never change direction and a draw that stays at the initial point: asserted here on all four runs' rows."""
    _, _, st_o, wp = oracle_run(dens, dim)
    shapes = tree_shapes(dens, dim, st_o, wp, 10)
    for build in ("general", "sampling"):
        want = {"turn@1", "turn@2", "turn@3", "top_uturn"}
        assert shapes[build] >= want, f"{build} build: the oracle's rows do not show {sorted(want - shapes[build])}"
    for md in (1, 2, 3):
        _, _, st_m, wp_m = oracle_run(dens, dim, maxdepth=md)
        for build, found in tree_shapes(dens, dim, st_m, wp_m, md).items():
            shapes[build] |= found
    for build in ("general", "sampling"):
        assert shapes[build] >= ALL_SHAPES, f"{build} build: the oracle's rows do not show {sorted(ALL_SHAPES - shapes[build])}"
    assert (st_o["transformation_update_id"][:NUM_TUNE] >= 0).any(), "the warm-up has no mass-matrix update"
    check_case(dens, dim)


@pytest.mark.parametrize("maxdepth", [1, 2, 3])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_depth_limit(oracle, dens, dim, maxdepth):
    """maxdepth 1, 2, 3: the draw ends right after the doubling that would have handed its end point to the next one; at maxdepth >= 2 trees
    with and without a change of direction on both builds"""
    _, _, st_o, wp = oracle_run(dens, dim, maxdepth=maxdepth)
    assert (st_o["depth"] <= maxdepth).all()
    shapes = tree_shapes(dens, dim, st_o, wp, maxdepth)
    for lo, hi, build in ((0, N_GENERAL, "general"), (N_GENERAL, N_DRAWS, "sampling")):
        assert (st_o["maxdepth_reached"][lo:hi] != 0).any(), f"{build} build: no draw reaches the depth limit"
        want = {"straight"} | {f"turn@{k}" for k in range(1, maxdepth)} if maxdepth >= 2 else set()
        assert shapes[build] >= want, f"{build} build: the oracle's rows do not show {sorted(want - shapes[build])}"
    check_case(dens, dim, maxdepth=maxdepth)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dens", DENS)
def test_extra_doublings(oracle, dens, dim):
    """extra_doublings 2: after a U-turn the tree is extended twice more in the direction of the doubling that turned, without tests"""
    _, _, st_o, _ = oracle_run(dens, dim, extra_doublings=2)
    for lo, hi, build in ((0, N_GENERAL, "general"), (N_GENERAL, N_DRAWS, "sampling")):
        # (a draw ends at the depth limit, on a divergence or on a U-turn: one that ended below the limit without a divergence turned, and
        # its last doublings are the extra ones)
        rows = st_o[lo:hi]
        assert ((rows["diverging"] == 0) & (rows["depth"] < 10) & (rows["depth"] >= 3)).any(), f"{build} build: no tree was extended after a U-turn"
    check_case(dens, dim, extra_doublings=2)


def test_without_turning_tests(oracle):
    """check_turning off: no U-turn test at any level, every tree runs to the depth limit (4 here) on both builds"""
    _, _, st_o, wp = oracle_run("iid", 513, check_turning=False, maxdepth=4)
    assert ((st_o["depth"] == 4) | (st_o["diverging"] != 0)).all() and (st_o["depth"] == 4).any()
    shapes = tree_shapes("iid", 513, st_o, wp, 4)
    for build in ("general", "sampling"):
        assert shapes[build] & {"turn@1", "turn@2", "turn@3"}, f"{build} build: no tree changes direction"
    check_case("iid", 513, check_turning=False, maxdepth=4)


def test_divergence_discards_a_doubling(oracle):
    """max_energy_error small enough that leaves diverge: the doubling in progress is discarded and the draw is taken from the tree before
    it — on both builds, after doublings that had already moved an end point"""
    kw = dict(max_energy_error=0.5)
    _, _, st_o, _ = oracle_run("diag", 1024, **kw)
    for lo, hi, build in ((0, N_GENERAL, "general"), (N_GENERAL, N_DRAWS, "sampling")):
        rows = st_o[lo:hi]
        hit = (rows["diverging"] != 0) & (rows["depth"] >= 1) & (rows["n_steps"] > (1 << rows["depth"].astype(np.int64)) - 1)
        assert hit.any(), f"{build} build: no divergence inside a doubling that follows a complete one"
        assert (rows["diverging"] == 0).any(), f"{build} build: every draw diverges"
    check_case("diag", 1024, **kw)
