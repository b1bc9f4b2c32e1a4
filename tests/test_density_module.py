"""User densities as modules (include/nuts_amd.h "User densities"; the device-side answer to the reference's `CpuLogpFunc`,
src/math/cpu_math.rs:885-970): a functor written against the kernel headers, compiled into its own shared object and
selected with NM_LOGP_MODULE.  The CPU test builds the module (hipcc cross-compiles) and checks its exports; the GPU test
runs it against the built-in density it re-implements and against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import build as B
from helpers import assert_bit_exact, run_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "user_density", "my_diag_normal.hpp")
MODDIR = os.path.join(HERE, "_modules")
DIM = 40


def module_path(dim=DIM):
    dpl, w = B.pick_tiling(dim) if dim <= 4096 else ("wide16", 4)
    return os.path.join(MODDIR, f"my_diag_normal_dpl{dpl}_w{w}.so")


def ensure_module(dim=DIM, group=False, lane=False):
    out = module_path(dim) if not (group or lane) else os.path.join(MODDIR, f"my_diag_normal_{'lane' if lane else 'group'}_dim{dim}.so")
    srcs = [HEADER] + [os.path.join(B.CSRC, f) for f in ("density_module.hip", "nuts_contract.hpp", "nuts_kernels.hpp", "nuts_launch.hpp", "dev_math.hpp",
                                                          "nuts_group.hpp", "nuts_group_impl.hpp", "nuts_lane.hpp", "nuts_adapt.hpp")]
    srcs.append(os.path.join(HERE, "..", "include", "nuts_amd.h"))       # the ABI version is part of the module
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        os.makedirs(MODDIR, exist_ok=True)
        B.build_density_module(HEADER, "MyDiagNormal", dim, out, group_struct="MyDiagNormalGroup" if (group or lane) else None,
                               lane_struct="MyDiagNormalLane" if lane else None)
    return out


def test_module_builds_and_exports():
    path = ensure_module()
    m = C.CDLL(path)
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert info[1] == N.load_library().nm_abi_version() and (info[2], info[3]) == B.pick_tiling(DIM) == (2, 1)
    assert info[4] == 0                                             # built without a group form
    assert hasattr(m, "nm_module_launch")
    L = N.load_library()
    d, w = C.c_uint64(), C.c_uint64()
    for dim in (1, 128, 129, 1024, 1025, 4096):                     # the Python table is the library's
        assert L.nm_pick_tiling(dim, 0, 0, C.byref(d), C.byref(w)) == 0 and (d.value, w.value) == B.pick_tiling(dim)
    assert L.nm_pick_tiling(4097, 0, 0, C.byref(d), C.byref(w)) == 4


@pytest.mark.gpu
def test_user_density_module_matches_builtin_and_oracle(oracle):
    path = ensure_module()
    prec = np.exp(np.random.default_rng(3).uniform(-3, 3, DIM))
    s = N.DiagNutsSettings(num_chains=5, seed=77, num_tune=80)
    x0 = oracle.init_positions_uniform(77, 0, 5, DIM)
    out = {}
    for name, logp in (("module", N.LogpSpec.module(DIM, path, prec)), ("builtin", N.LogpSpec.diag_normal(prec))):
        b = N.ChainBatch(s, logp, 5)
        b.set_position(x0)
        out[name] = b.draw_many(140)
        b.close()
    assert (out["module"][0].view(np.uint64) == out["builtin"][0].view(np.uint64)).all()
    pos_o, st_o, _, failed = run_oracle(oracle, s, N.LogpSpec.diag_normal(prec), 5, x0, 140)
    assert failed == 0
    assert_bit_exact(out["module"][0], out["module"][1], pos_o, st_o)
    # a module is tied to one tiling: the engine says so instead of launching the wrong kernel
    with pytest.raises(N.NutsAmdError) as e:
        N.ChainBatch(s, N.LogpSpec.module(200, path, np.ones(200)), 5)
    assert e.value.status == 1 and "tiling" in str(e.value)
    with pytest.raises(N.NutsAmdError) as e:
        N.ChainBatch(s, N.LogpSpec.module(DIM, os.path.join(HERE, "no_such_module.so"), prec), 5)
    assert e.value.status == 1 and "cannot load" in str(e.value)


GROUP_DIM = 10


def test_group_form_module_builds():
    m = C.CDLL(ensure_module(GROUP_DIM, group=True))
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert (info[2], info[3], info[4]) == (2, 1, 8)                 # 8 lanes per chain for dim <= 16


@pytest.mark.gpu
def test_user_density_group_form_matches_oracle(oracle):
    """A user density with a group form: its chains are drawn 8 per wavefront, with the oracle's bits."""
    path = ensure_module(GROUP_DIM, group=True)
    prec = np.exp(np.random.default_rng(4).uniform(-2, 2, GROUP_DIM))
    n = 37
    s = N.DiagNutsSettings(num_chains=n, seed=78, num_tune=70)
    x0 = oracle.init_positions_uniform(78, 0, n, GROUP_DIM)
    b = N.ChainBatch(s, N.LogpSpec.module(GROUP_DIM, path, prec), n, lane_groups=2)
    b.set_position(x0)
    pos, st = b.draw_many(120)
    assert b.group_launches() == 1
    b.close()
    pos_o, st_o, _, failed = run_oracle(oracle, s, N.LogpSpec.diag_normal(prec), n, x0, 120)
    assert failed == 0
    assert_bit_exact(pos, st, pos_o, st_o)
    # a module without a group form keeps one wavefront per chain, whatever lane_groups says
    b = N.ChainBatch(s, N.LogpSpec.module(DIM, ensure_module(), np.ones(DIM)), n, lane_groups=2)
    b.set_position(oracle.init_positions_uniform(78, 0, n, DIM))
    b.draw_many(5)
    assert b.group_launches() == 0
    b.close()


def test_lane_form_module_builds():
    m = C.CDLL(ensure_module(GROUP_DIM, lane=True))
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert (info[2], info[3], info[4], info[6]) == (2, 1, 8, 1) and hasattr(m, "nm_module_launch_lane")


@pytest.mark.gpu
def test_user_density_lane_form_matches_oracle(oracle):
    """A user density with a LANE form: its chains are drawn one per lane, 64 per wavefront, with the
    oracle's bits — the one-chain-per-lane kernels are no longer reserved for the built-in densities."""
    path = ensure_module(GROUP_DIM, lane=True)
    prec = np.exp(np.random.default_rng(4).uniform(-2, 2, GROUP_DIM))
    n = 150
    s = N.DiagNutsSettings(num_chains=n, seed=79, num_tune=70)
    x0 = oracle.init_positions_uniform(79, 0, n, GROUP_DIM)
    b = N.ChainBatch(s, N.LogpSpec.module(GROUP_DIM, path, prec), n, lane_chains=2)
    b.set_position(x0)
    pos, st = b.draw_many(120)
    assert b.lane_launches() >= 1 and b.group_launches() == 0
    b.close()
    pos_o, st_o, _, failed = run_oracle(oracle, s, N.LogpSpec.diag_normal(prec), n, x0, 120)
    assert failed == 0
    assert_bit_exact(pos, st, pos_o, st_o)


def ensure_variant_module(dim=DIM):
    out = os.path.join(MODDIR, f"my_diag_normal_variants_dim{dim}.so")
    srcs = [HEADER] + [os.path.join(B.CSRC, f) for f in ("density_module.hip", "nuts_contract.hpp", "nuts_kernels.hpp", "nuts_launch.hpp", "dev_math.hpp")]
    srcs.append(os.path.join(HERE, "..", "include", "nuts_amd.h"))
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        os.makedirs(MODDIR, exist_ok=True)
        B.build_density_module(HEADER, "MyDiagNormal", dim, out, variants=("low_rank", "kinetic"))
    return out


def test_variant_module_builds():
    m = C.CDLL(ensure_variant_module())
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert info[7] == 3 and hasattr(m, "nm_module_launch_variant")
    m0 = C.CDLL(ensure_module())
    m0.nm_module_info(info)
    assert info[7] == 0


@pytest.mark.gpu
def test_user_density_with_low_rank_adaptation_trajectory_kinds_and_mclmc(oracle):
    """VERDICT r03 "missing" 3 / 4: a user density module behind `LowRankNutsSettings` (adapting, the estimator on the device), behind
    the ExactNormal and Microcanonical trajectory kinds and behind MCLMC — the module carries the LrWrap / KinWrap kernels when built
    with NM_MODULE_VARIANTS.  Each run is bit-identical to the built-in density it re-implements and to the oracle."""
    from nuts_rs_amd import _lib
    from helpers import oracle_settings
    path = ensure_variant_module()
    prec = np.exp(np.random.default_rng(5).uniform(-3, 3, DIM))
    n = 4
    cases = [("low_rank", N.LowRankNutsSettings(num_chains=n, seed=81, num_tune=120), 150),
             ("exact_normal", N.DiagNutsSettings(num_chains=n, seed=82, num_tune=60, trajectory_kind=N.KineticEnergyKind.EXACT_NORMAL), 90),
             ("microcanonical", N.DiagNutsSettings(num_chains=n, seed=83, num_tune=60, trajectory_kind=N.KineticEnergyKind.MICROCANONICAL), 90),
             ("low_rank_microcanonical", N.LowRankNutsSettings(num_chains=n, seed=84, num_tune=100, trajectory_kind=N.KineticEnergyKind.MICROCANONICAL), 120),
             ("mclmc", N.DiagMclmcSettings(num_chains=n, seed=85, num_tune=60, step_size=0.5, momentum_decoherence_length=3.0), 90)]
    for name, s, draws in cases:
        x0 = oracle.init_positions_uniform(s.seed, 0, n, DIM)
        out = {}
        for which, logp in (("module", N.LogpSpec.module(DIM, path, prec)), ("builtin", N.LogpSpec.diag_normal(prec))):
            b = N.ChainBatch(s, logp, n)
            b.set_position(x0)
            out[which] = b.draw_many(draws)
            tpc = b.threads_per_chain()
            if "low_rank" in name:
                assert b.lowrank_device_updates() >= n * 3
            b.close()
        assert (out["module"][0].view(np.uint64) == out["builtin"][0].view(np.uint64)).all(), name
        est = dict(estimator=C.cast(_lib.load().nm_lowrank_block_twin, oracle.ESTIMATOR_FN)) if "low_rank" in name else {}
        pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, s), N.LogpSpec.diag_normal(prec).kind, DIM, prec, oracle.gpu_cfg(tpc), n, x0, draws, **est)
        assert failed == 0, name
        assert_bit_exact(out["module"][0], out["module"][1], pos_o, st_o)
    # a module built without the variants says so
    plain = ensure_module()
    for s in (N.LowRankNutsSettings(num_chains=n, seed=1, num_tune=20),
              N.DiagNutsSettings(num_chains=n, seed=1, num_tune=20, trajectory_kind=N.KineticEnergyKind.EXACT_NORMAL)):
        with pytest.raises(N.NutsAmdError) as e:
            N.ChainBatch(s, N.LogpSpec.module(DIM, plain, prec), n)
        assert e.value.status == 4 and "NM_MODULE_VARIANTS" in str(e.value)


def ensure_group_variant_module():
    out = os.path.join(MODDIR, f"my_diag_normal_group_kinetic_dim{GROUP_DIM}.so")
    srcs = [HEADER] + [os.path.join(B.CSRC, f) for f in ("density_module.hip", "nuts_contract.hpp", "nuts_kernels.hpp", "nuts_launch.hpp", "dev_math.hpp", "nuts_group.hpp", "nuts_group_impl.hpp", "nuts_adapt.hpp")]
    srcs.append(os.path.join(HERE, "..", "include", "nuts_amd.h"))
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        os.makedirs(MODDIR, exist_ok=True)
        B.build_density_module(HEADER, "MyDiagNormal", GROUP_DIM, out, group_struct="MyDiagNormalGroup", variants=("kinetic",))
    return out


def test_group_form_module_with_kinetic_variant_builds():
    m = C.CDLL(ensure_group_variant_module())
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert (info[4], info[7]) == (8, 2)


@pytest.mark.gpu
def test_user_density_group_form_with_trajectory_kinds_and_mclmc(oracle):
    """A user density with a group form AND the kinetic variant: the ExactNormal / Microcanonical kinds and MCLMC run 8 chains per wavefront
    on it, with the oracle's bits (the group kernels' kinds, nuts_group_impl.hpp, through the module mechanism)."""
    path = ensure_group_variant_module()
    prec = np.exp(np.random.default_rng(6).uniform(-2, 2, GROUP_DIM))
    n = 37
    for s, draws in ((N.DiagNutsSettings(num_chains=n, seed=91, num_tune=60, trajectory_kind=N.KineticEnergyKind.EXACT_NORMAL), 100),
                     (N.DiagNutsSettings(num_chains=n, seed=92, num_tune=60, trajectory_kind=N.KineticEnergyKind.MICROCANONICAL), 100),
                     (N.DiagMclmcSettings(num_chains=n, seed=93, num_tune=60, step_size=0.5), 100)):
        x0 = oracle.init_positions_uniform(s.seed, 0, n, GROUP_DIM)
        b = N.ChainBatch(s, N.LogpSpec.module(GROUP_DIM, path, prec), n, lane_groups=2)
        b.set_position(x0)
        pos, st = b.draw_many(draws)
        assert b.group_launches() >= 1
        b.close()
        pos_o, st_o, _, failed = run_oracle(oracle, s, N.LogpSpec.diag_normal(prec), n, x0, draws)
        assert failed == 0
        assert_bit_exact(pos, st, pos_o, st_o)


WALLED = os.path.join(HERE, "user_density", "my_walled_normal.hpp")


def ensure_walled(dim):
    dpl, w = B.pick_tiling(dim)
    out = os.path.join(MODDIR, f"my_walled_normal_dpl{dpl}_w{w}.so")
    srcs = [WALLED] + [os.path.join(B.CSRC, f) for f in ("density_module.hip", "nuts_contract.hpp", "nuts_kernels.hpp", "nuts_launch.hpp", "dev_math.hpp")]
    srcs.append(os.path.join(HERE, "..", "include", "nuts_amd.h"))
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        os.makedirs(MODDIR, exist_ok=True)
        B.build_density_module(WALLED, "MyWalledNormal", dim, out)
    return out


def test_fallible_module_builds():
    assert os.path.exists(ensure_walled(24))


@pytest.mark.gpu
def test_fallible_user_density_matches_oracle(oracle):
    """A device density with an error return (`kCanFail`, `status`): a recoverable error is a divergence without an energy
    error, an unrecoverable one stops the chain — draw for draw what the oracle's chain does with a host function that applies
    the same rules around the same arithmetic (the oracle's own N(mu, I) in the engine's reduction order)."""
    import ctypes
    dim, n, tune, draws = 24, 8, 60, 140
    mu, wall1, wall2 = 0.5, 2.0, 3.1
    path = ensure_walled(dim)
    s = N.DiagNutsSettings(num_chains=n, seed=123, num_tune=tune, store_divergences=True)
    x0 = oracle.init_positions_uniform(s.seed, 0, n, dim)
    b = N.ChainBatch(s, N.LogpSpec.module(dim, path, np.array([mu, wall1, wall2])), n, lane_groups=1)
    status = b.set_position(x0, raise_on_error=False)
    pos, st = b.draw_many(draws, raise_on_error=False)
    tpc = b.threads_per_chain()
    b.close()
    cfg = oracle.gpu_cfg(tpc)
    L = oracle.lib()
    par = np.array([mu])
    g_buf = np.zeros(dim)

    def tramp(ctx, d, px, pg, plogp):
        x = np.ctypeslib.as_array(px, shape=(d,))
        if x[1] > wall2:
            return 2
        if x[0] > wall1:
            return 1
        out = ctypes.c_double()
        rc = L.nmo_logp(ctypes.byref(cfg), oracle.LOGP_IID_NORMAL, d, par, 1, np.ascontiguousarray(x), g_buf, ctypes.byref(out))
        np.ctypeslib.as_array(pg, shape=(d,))[:] = g_buf
        plogp[0] = out.value
        return rc
    cb = oracle.HOST_LOGP_FN(tramp)
    so = oracle_settings_for(oracle, s)
    stopped = 0
    for c in range(n):
        ch = oracle.Chain(so, 0, dim, np.zeros(1), cfg, chain_id=c, callback=cb)
        assert ch.set_position(x0[c]) == int(status[c]) == 0
        for t in range(draws):
            p, q, rc = ch.draw()
            assert int(st["chain_status"][t, c]) == rc, (c, t)
            if rc != 0:
                stopped += 1
                break
            assert (p.view(np.uint64) == pos[t, c].view(np.uint64)).all(), (c, t)
            for f in ("depth", "n_steps", "diverging", "step_size", "energy", "logp", "mean_tree_accept"):
                assert q[f] == st[f][t, c], (f, c, t)
            a, bb = q["divergence_energy_error"], st["divergence_energy_error"][t, c]
            assert (np.isnan(a) and np.isnan(bb)) or a == bb
    div = st["diverging"] != 0
    assert div.sum() > 3 and np.isnan(st["divergence_energy_error"][div]).any()     # the recoverable wall was met
    assert stopped >= 1, "no chain met the fatal wall: move it"


def oracle_settings_for(oracle, s):
    from helpers import oracle_settings
    return oracle_settings(oracle, s)


WIDE_DIM = 6000


def test_wide_chain_module_builds():
    m = C.CDLL(ensure_module(WIDE_DIM))
    info = (C.c_uint64 * 8)()
    m.nm_module_info(info)
    assert (info[2], info[3], info[5]) == (16, 4, 1)                 # the (16, 4) tiling, built for several blocks per chain


@pytest.mark.gpu
def test_wide_chain_user_density_matches_builtin_and_oracle(oracle):
    """A fused USER density for a chain wider than one block (dim > 4096): the module is compiled in cluster mode and brings
    `init_slice`; same bits as the built-in diagonal normal and as the oracle."""
    from helpers import oracle_settings
    path, n, draws = ensure_module(WIDE_DIM), 3, 36
    prec = np.exp(np.random.default_rng(4).uniform(-2, 2, WIDE_DIM))
    s = N.DiagNutsSettings(num_chains=n, seed=78, num_tune=24)
    x0 = oracle.init_positions_uniform(78, 0, n, WIDE_DIM)
    out = {}
    for name, logp in (("module", N.LogpSpec.module(WIDE_DIM, path, prec)), ("builtin", N.LogpSpec.diag_normal(prec))):
        b = N.ChainBatch(s, logp, n)
        assert b.blocks_per_chain() == 2
        b.set_position(x0)
        out[name] = b.draw_many(draws)
        b.close()
    assert (out["module"][0].view(np.uint64) == out["builtin"][0].view(np.uint64)).all()
    pos_o, st_o, _, failed = oracle.run(oracle_settings(oracle, s), oracle.LOGP_DIAG_NORMAL, WIDE_DIM, prec, oracle.gpu_cfg(256, gpu_slice=4096), n, x0, draws, n_threads=8)
    assert failed == 0
    assert_bit_exact(out["module"][0], out["module"][1], pos_o, st_o)
    with pytest.raises(N.NutsAmdError) as e:                        # a one-block module cannot serve a wide chain, and vice versa
        N.ChainBatch(s, N.LogpSpec.module(WIDE_DIM, ensure_module(), prec), n)
    assert "wide chains" in str(e.value)
    with pytest.raises(N.NutsAmdError) as e:
        N.ChainBatch(s, N.LogpSpec.module(DIM, path, prec[:DIM]), n)
    assert "wide chains" in str(e.value)
