"""Which kernel family serves an engine, pinned: tests/golden/engine_selection_parent.json holds, for every case, the inputs (density,
settings, chain count, nm_engine_config, the calls made) and what the library's accessors reported after each call on the commit BEFORE
the selection moved into csrc/engine_plan.hpp.  This test replays the file on the built library and compares field by field: the
returned status of every call, the tiling, the grids, every launch counter and the reduction order.  The grids depend on the device's
compute-unit count, which the file records: on another device the test FAILS (it does not skip) and says to record the file again.

`run_case` is the whole interpreter of a case; recording the file is `run_case` on every case's inputs.  The file keeps one case per
line and what a call left behind as a list of values in the order of its "observed_fields" (the call's status, then ACCESSORS)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nuts_rs_amd as N
from nuts_rs_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "engine_selection_parent.json")

ACCESSORS = ("nm_engine_threads_per_chain", "nm_engine_dims_per_lane", "nm_engine_blocks_per_chain", "nm_debug_group_grid",
             "nm_debug_group_roomy_launches", "nm_debug_sampling_launches", "nm_engine_group_launches", "nm_engine_lane_launches",
             "nm_engine_tile_launches", "nm_engine_lockstep_launches", "nm_engine_reduce_order")
SETTINGS_BASE = {"diag": "nm_settings_default", "low_rank": "nm_settings_default_low_rank", "mclmc": "nm_settings_default_mclmc"}


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _logp(spec):
    kind, dim = spec["kind"], int(spec.get("dim", 0))
    if kind == "iid_normal":
        return N.LogpSpec.iid_normal(dim, 3.0)
    if kind == "diag_normal":
        return N.LogpSpec.diag_normal(np.ones(dim))
    if kind == "funnel":
        return N.LogpSpec.funnel(dim)
    if kind == "eight_schools":
        return N.LogpSpec.eight_schools()
    if kind == "mvn_prec":          # identity plus a constant: symmetric, positive definite
        return N.LogpSpec.mvn_precision(np.eye(dim) + 0.5 / dim)
    if kind == "host_callback":
        return N.LogpSpec.host_callback(dim, lambda chain, x: (-0.5 * float(x @ x), -x), threads=2)
    if kind == "module":            # tests/user_density/my_diag_normal.hpp, built as tests/test_density_module.py builds it
        from test_density_module import ensure_module
        path = ensure_module(dim, group=spec.get("form") == "group", lane=spec.get("form") == "lane")
        return N.LogpSpec.module(dim, path, np.ones(dim))
    raise ValueError(kind)


def _observe(L, h):
    out = []
    for name in ACCESSORS:
        fn = getattr(L, name)
        fn.argtypes, fn.restype = [C.c_void_p], C.c_uint64
        out.append(int(fn(h)))
    return out


def run_case(case):
    """Create the case's engine and make its calls; -> {"create": status, "after_create": [values of ACCESSORS], "calls": [[status, values of ACCESSORS] per call]}."""
    L = N.load_library()
    s = _lib.NmSettings()
    getattr(L, SETTINGS_BASE[case["settings"].get("base", "diag")])(C.byref(s))
    for k, v in case["settings"].items():
        if k != "base":
            setattr(s, k, v)
    cfg = _lib.NmEngineConfig()
    L.nm_engine_config_default(C.byref(cfg))
    for k, v in case.get("config", {}).items():
        setattr(cfg, k, v)
    logp = _logp(case["logp"])
    cl = logp.to_c()
    n, dim = int(case["n_chains"]), logp.dim
    h = C.c_void_p()
    obs = {"create": int(L.nm_engine_create(C.byref(s), C.byref(cl), n, C.byref(cfg), C.byref(h))), "calls": []}
    if obs["create"] != 0:
        return obs
    try:
        obs["after_create"] = _observe(L, h)
        for call in case["calls"]:
            if call[0] == "set_positions":
                x0 = np.empty((n, dim))
                _lib.check(L.nm_init_positions_uniform(s.seed, 0, n, dim, x0.ctypes.data))
                st = L.nm_engine_set_positions(h, x0.ctypes.data, None)
            elif call[0] == "draw":
                st = L.nm_engine_draw(h, int(call[1]), None, None)
            elif call[0] == "set_transform":        # one transformation for all chains: unit scales, the first `rank` unit vectors
                rank = int(call[1])
                stds, mean, mu = np.ones(dim), np.zeros(dim), np.zeros(dim)
                vals, vecs = np.full(rank, 2.0), np.ascontiguousarray(np.eye(dim)[:rank])
                st = L.nm_engine_set_transform(h, 0, rank, stds.ctypes.data, mean.ctypes.data, vals.ctypes.data, vecs.ctypes.data, mu.ctypes.data)
            else:
                raise ValueError(call)
            obs["calls"].append([int(st)] + _observe(L, h))
    finally:
        L.nm_engine_synchronize(h)
        L.nm_engine_destroy(h)
    return obs


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _cases():
    return [pytest.param(c, id=c["name"]) for c in _golden()["cases"]] if os.path.exists(GOLDEN) else []


def test_the_recorded_cases_are_there():
    g = _golden()
    assert g["observed_fields"] == ["status"] + list(ACCESSORS)
    assert g["cu_count"] > 0 and len(g["cases"]) >= 60 and len({c["name"] for c in g["cases"]}) == len(g["cases"])
    for c in g["cases"]:
        assert len(c["observed"]["calls"]) == (len(c["calls"]) if c["observed"]["create"] == 0 else 0), c["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases())
def test_engine_selection_is_the_parents(case):
    want_cus = _golden()["cu_count"]
    assert cu_count() == want_cus, (f"this device has {cu_count()} compute units, tests/golden/engine_selection_parent.json was recorded on {want_cus}: "
                                    "the grids differ; record the file again on this device AT THE PARENT COMMIT of the change under test")
    got, want = run_case(case), case["observed"]
    assert got["create"] == want["create"], (case["name"], "nm_engine_create", got["create"], want["create"])
    assert len(got["calls"]) == len(want["calls"])
    rows = [("after nm_engine_create", ACCESSORS, got.get("after_create", []), want.get("after_create", []))]
    rows += [(f"call {i} {case['calls'][i]}", ("status",) + ACCESSORS, g, w) for i, (g, w) in enumerate(zip(got["calls"], want["calls"]))]
    for where, fields, g, w in rows:
        assert len(g) == len(w)
        for k, gv, wv in zip(fields, g, w):
            assert gv == wv, (case["name"], where, k, gv, wv)
