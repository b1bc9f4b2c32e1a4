"""The case lists of tests/test_gpu_vector_outputs.py are the product they claim to be, `plan_engine` / `plan_draw` (csrc/engine_plan.hpp) name
for every case the kernel family its GPU test asserts, and the oracle's per-chain `Chain.draw(vectors=...)` gives the rows of
`oracle.run(vectors=...)` (no GPU needed)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from nuts_rs_amd import selftest_cases as SC

import test_gpu_vector_outputs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vector_plan_check.hip")
EXE = os.path.join(ROOT, "tests", "cpp", "vector_plan_check")
CSRC = os.path.join(ROOT, "nuts_rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CAPS = {(d, w): d * 64 * w for (d, w) in SC.TILINGS}


def test_every_family_and_unique_ids():
    cases = V.all_cases()
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    assert {c["fam"] for c in cases} == set("ABCDEFG")
    assert all(c["id"].startswith(c["fam"] + "-") for c in cases)
    for c in cases:
        assert set(c["conds"]) <= set(V.CONDITIONS) and "tune" in c["conds"], c["id"]
        assert c["cut"] % 2 == 1 and 0 < c["cut"] < c["draws"] and c["tune"] < c["draws"], c["id"]
        d, w = c["tiling"]
        assert c["dim"] <= CAPS[(d, w)] or c["served"] == "cluster", c["id"]
        assert 0 <= c["seed"] < 32, c["id"]                       # what tools/small_chain_dry_run.py --only vectors scans
    assert set(V.SEEDS) <= set(ids)


def test_family_a_is_every_tiling_at_both_dims():
    a = [c for c in V.all_cases() if c["fam"] == "A"]
    dims = V.tiling_dims()
    assert list(dims) == SC.TILINGS and len(dims) == 8
    for (d, w), (ragged, full) in dims.items():
        lower = max([0] + [cap for cap in CAPS.values() if cap < CAPS[(d, w)]])
        assert full == CAPS[(d, w)] and ragged % 2 == 1 and lower < ragged < full
        assert ragged == (lower + 1 if lower else 125)              # just above the previous capacity; (2,1): the iid rows' ragged top
        iid_rows = {c["dim"] for c in SC.cases() if c["dens"] == "iid" and (c["dpl"], c["w"]) == (d, w)}
        assert ragged in iid_rows
    diag = {(c["tiling"], c["dim"]) for c in a if c["dens"] == "diag"}
    assert diag == {(t, dim) for t, pair in dims.items() for dim in pair} and len(diag) == 16
    for c in a:
        assert c["kind"] == "nuts" and not c["lr"] and c["engine"] == V.ONE_CHAIN and c["served"] == "wave"
        assert set(c["conds"]) == set(V.NUTS_CONDS)                 # no condition dropped
        if c["dens"] == "diag":
            assert c["skw"] == dict(max_energy_error=0.25)
    assert {c["tiling"] for c in a if c["dens"] == "funnel"} == {(2, 1), (4, 1)}
    assert [(c["tiling"], c["engine"]["chain_tiles"]) for c in a if c["dens"] == "mvn"] == [((4, 1), 1)]


def test_every_kind_in_c_d_f_and_the_other_families_shapes():
    cases = V.all_cases()
    by = lambda f: [c for c in cases if c["fam"] == f]
    kinds = {"exact", "micro", "mclmc"}
    assert {(c["kind"], c["tiling"]) for c in by("C")} == {(k, t) for k in kinds for t in ((16, 1), (4, 4))}
    assert all(c["dim"] % (64 * 16) != 0 for c in by("C") if c["tiling"] == (16, 1))            # ragged
    assert [c["skw"]["dynamic_step_size"] for c in by("C") if c["id"].endswith("-ladder")] == [True]
    assert {c["kind"] for c in by("D")} == kinds | {"nuts"}
    assert {(c["dens"], c["dim"]) for c in by("D") if c["kind"] == "nuts"} == {(d, n) for d in ("iid", "diag") for n in (4097, 8193)}
    assert all(c["chains"] == 2 and c["served"] == "cluster" for c in by("D"))
    assert [c["dim"] for c in by("D") if c["env"]] == [8193] and [c["env"] for c in by("D") if c["env"]] == [dict(NM_CLUSTER_GENERAL="1")]
    f = by("F")
    assert {c["kind"] for c in f if c["served"] == "group"} == kinds
    assert sorted((c["dim"], c["chains"]) for c in f if c["served"] == "group") == [(11, 21), (30, 9), (50, 5)]
    for c in f:
        if c["served"] == "group":                                  # 8 / 4 / 2 chains per wavefront, the last wavefront partly filled
            per_wave = 64 // (8 if c["dim"] <= 16 else 16 if c["dim"] <= 32 else 32)
            assert c["chains"] % per_wave != 0
    assert sorted((c["kind"], c["dim"]) for c in f if c["served"] == "lane") == [("exact", 10), ("micro", 3)]
    assert all(c["chains"] % 64 != 0 for c in f if c["served"] == "lane")
    # (the one-chain-per-lane kernels have no MCLMC form: engine_plan.hpp lane_kin_ok)
    e = by("E")
    assert {c["tiling"] for c in e if c["dens"] == "hostcb" and c["kind"] == "nuts" and not c["lr"] and c["served"] == "wave"} == {(2, 1), (4, 4), (16, 4)}
    assert {c["tiling"] for c in e if c["dens"] == "hostcb_wall"} == {(2, 1), (16, 4)}
    assert any(c["lr"] == "hostcb" for c in e) and any(c["kind"] == "micro" for c in e) and [c["dim"] for c in e if c["served"] == "cluster"] == [4500]
    assert all(c["dim"] % (64 * 16 * 4) != 0 for c in e if c["tiling"] == (16, 4))              # ragged
    b = by("B")
    assert {c["tiling"] for c in b if c["lr"] == "adapt"} == {(2, 1), (8, 2)} and [c["dim"] for c in b if c["tiling"] == (8, 2)] == [300]
    shared = {(c["served"], c["engine"]["chain_tiles"], c["order"], c["dim"], c["rank"], c["chains"]) for c in b if c["lr"] == "shared"}
    assert shared == {(s, t, o, *shape) for (s, t, o) in (("tile", 2, 1), ("tile", 0, 1), ("lockstep", 3, 2)) for shape in ((64, 16, 21), (200, 200, 16))}
    assert all(tuple(c["vectors"]) == V.LOCKSTEP_VECTORS for c in b if c["served"] == "lockstep")
    assert [(c["dim"], c["rank"]) for c in b if c["lr"] == "per_chain"] == [(70, 3)]
    g = by("G")
    assert [c["tiling"] for c in g] == [(2, 1), (16, 1)] and g[1]["cut"] > g[1]["tune"] + 1     # the second launch: the sampling build alone
    # no family drops a condition in all of its cases unless it cannot produce the event
    for fam in "ABCDEFG":
        kept = set().union(*(set(c["conds"]) for c in by(fam)))
        assert {"mm", "tune", "stay", "move"} <= kept, fam
        assert {"div0", "divN"} <= kept, fam


def test_inputs_are_exact_and_index_dependent():
    p = V.index_precisions(300)
    assert len(set(p[:40])) == 40 and (np.frexp(p)[0] * 16 == np.round(np.frexp(p)[0] * 16)).all()
    for dim, rank in ((64, 16), (200, 200), (70, 3)):
        stds, mean, vals, vecs, mu = V.exact_transform(dim, rank, 7 + dim)
        assert vecs.shape == (rank, dim) and (vecs @ vecs.T == np.eye(rank)).all()           # orthonormal, exactly
        assert (stds > 0).all() and (vals > 0).all()
    t = V.exact_transform(70, 3, 77, per_chain=3)
    assert t[3].shape == (3, 3, 70) and not (t[0][0] == t[0][1]).all()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc compiles the host harness (engine_plan.hpp includes dev_math.hpp)")
def test_plan_engine_selects_the_family_the_gpu_case_asserts():
    deps = [SRC, os.path.join(ROOT, "include", "nuts_amd.h")] + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", SRC, "-o", EXE])
    cases = V.all_cases()
    lines = []
    for c in cases:
        s = V.make_settings(c).to_c()
        kw = V.engine_kwargs(c)
        tr = {None: 0, "adapt": 0, "shared": 1, "hostcb": 1, "per_chain": 2}[c["lr"]]
        lines.append(" ".join(str(int(x)) if not isinstance(x, str) else x for x in (
            c["id"], V.make_logp(c).kind, c["dim"], c["chains"], kw.get("dims_per_lane", 0), kw.get("waves_per_chain", 0), kw.get("lane_groups", 0),
            kw.get("lane_chains", 0), kw.get("chain_tiles", 0), s.adaptation, s.freeze_transform, s.trajectory_kind, s.sampler, s.num_tune, s.maxdepth,
            s.store_divergences, s.store_mass_matrix, tr, c["rank"], c["cut"], c["draws"])))
    r = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().split("\n")}
    assert set(out) == {c["id"] for c in cases}
    family = {"wave": {(False, False): 0, (True, False): 1, (False, True): 2}, "cluster": {(False, False): 3, (False, True): 4}}
    for c in cases:
        status, fam, dpl, wpc, cl_k, *served = out[c["id"]]
        assert status == "0", (c["id"], out[c["id"]])
        d, w = c["tiling"]
        assert (int(dpl), int(wpc)) == (d, w), c["id"]
        kin = c["kind"] != "nuts"
        want_family = (family["cluster"][(False, kin)] if c["served"] == "cluster" else 1 if c["lr"] else 2 if kin else 0)
        assert int(fam) == want_family, (c["id"], fam)
        assert int(cl_k) == (-(-c["dim"] // 4096) if c["served"] == "cluster" else 1), c["id"]
        sampling = (c["served"] == "wave" and c["kind"] == "nuts" and not c["lr"] and w == 1 and d in (8, 16) and not c["dens"].startswith("hostcb"))
        want = {"wave": ["wave"], "cluster": ["wave"], "group": ["group"], "lane": ["lane"], "tile": ["tile"], "lockstep": ["lockstep"]}[c["served"]]
        if sampling:
            want = ["sampling", "wave"]                                   # the draws up to num_tune on the general kernel, the rest on the sampling build
        assert served == sorted(want), (c["id"], served)


def test_chain_draw_vectors_matches_run_vectors(oracle):
    """`Chain.draw(vectors=...)` (nmo_chain_draw_ex) against `oracle.run(vectors=...)` on a built-in density: the same rows, NaN for NaN."""
    O = oracle
    c = [x for x in V.all_cases() if x["id"] == "A-funnel-2x1-dim31"][0]
    o = V.oracle_side(O, c)
    assert V.findings(c, o["x0"], o["pos"], o["st"], o["vec"]) == [] and sorted(o["vec"]) == sorted(O.VECTOR_STATS)
    s, logp = V.make_settings(c), V.make_logp(c)
    so = V.oracle_settings(O, s)
    for k in range(c["chains"]):
        ch = O.Chain(so, logp.kind, logp.dim, logp.params, V.oracle_cfg(O, c), chain_id=k)
        assert ch.set_position(o["x0"][k]) == 0
        for t in range(c["draws"]):
            row = {}
            pos, st, rc = ch.draw(vectors=row)
            assert rc == 0 and sorted(row) == sorted(O.VECTOR_STATS)
            assert V.bits_equal(pos, o["pos"][t, k]).all() and st.tobytes() == o["st"][t, k].tobytes()
            for name in O.VECTOR_STATS:
                assert row[name].shape == (c["dim"],)
                assert (V.bits_equal(row[name], o["vec"][name][t, k]) | (np.isnan(row[name]) & np.isnan(o["vec"][name][t, k]))).all(), (name, t, k)
                assert (np.isnan(row[name]) == np.isnan(o["vec"][name][t, k])).all(), (name, t, k)
    # the plain form is unchanged: no vectors, the same draw
    ch = O.Chain(so, logp.kind, logp.dim, logp.params, V.oracle_cfg(O, c), chain_id=0)
    assert ch.set_position(o["x0"][0]) == 0
    pos, st, rc = ch.draw()
    assert rc == 0 and V.bits_equal(pos, o["pos"][0, 0]).all()
