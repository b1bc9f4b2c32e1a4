"""Oracle-only dry run (no GPU) of the case lists of tests/test_gpu_small_chain_instantiations.py and of
`test_instantiation_bit_exact_generic_inputs` (tests/test_gpu_every_instantiation.py): those tests skip nothing, so every case must be one in
which the oracle accepts every initial point and no sampled chain fails.  A case reported here gets another seed in the test file's
SEEDS / GENERIC_SEEDS.

    python tools/small_chain_dry_run.py [--cus 256] [--only small|generic]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import nuts_rs_amd as N  # noqa: E402
from helpers import oracle_settings  # noqa: E402
from oracle import oracle as O  # noqa: E402


def small(cus):
    import test_gpu_small_chain_instantiations as M
    bad, chains, div = [], 0, 0
    for c in M.group_cases() + M.lane_cases():
        n, _, offsets = M.chain_plan(c, cus)
        s = M.make_settings(c, n)
        logp = M.make_logp(c, s.seed)
        x0 = np.empty((n, c["dim"]))
        for off in offsets:                       # only the sampled chains' initial points
            w = min(M.WINDOW, n - off)
            x0[off:off + w] = O.init_positions_uniform(s.seed, off, w, c["dim"])
        ids, pos, st, failed = M.oracle_windows(O, c, s, logp, x0, offsets)
        chains += len(ids)
        div += int(st["diverging"].sum())
        if failed or not (st["chain_status"] == 0).all() or not np.isfinite(pos).all():
            bad.append(M.case_id(c))
    return len(M.group_cases()) + len(M.lane_cases()), chains, div, bad


def generic():
    import test_gpu_every_instantiation as E
    from nuts_rs_amd import selftest_cases as SC
    bad, chains, cases = [], 0, SC.cases(both_ends=False)
    for c in cases:
        r = E.generic_run(c)
        s, logp, transform, n = r["settings"], r["logp"], r["transform"], r["n_chains"]
        x0 = O.init_positions_uniform(s.seed, 0, n, logp.dim)
        est = {}
        if transform == "adapt":                  # the device estimator's twin lives in the engine's library (host code)
            from nuts_rs_amd import _lib
            transform, est = None, dict(estimator=C.cast(_lib.load().nm_lowrank_block_twin, O.ESTIMATOR_FN))
        tpc = 64 * (1 if c["dens"] == "schools" else c["w"])
        pos, st, _, failed = O.run(oracle_settings(O, s), logp.kind, logp.dim, logp.params, O.gpu_cfg(tpc), n, x0, r["draws"], n_threads=8,
                                   transform=transform, **est)
        chains += n
        if failed or not (st["chain_status"] == 0).all() or not np.isfinite(pos).all():
            bad.append(SC.case_id(c))
    return len(cases), chains, bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--only", choices=["small", "generic"])
    a = ap.parse_args()
    O.lib()
    rc = 0
    if a.only != "generic":
        t = time.time()
        n, chains, div, bad = small(a.cus)
        print(f"small-chain matrix: {n} cases, {chains} oracle chains, {div} divergent draws, {len(bad)} cases with a failed chain {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    if a.only != "small":
        t = time.time()
        n, chains, bad = generic()
        print(f"generic inputs: {n} cases, {chains} oracle chains, {len(bad)} cases with a failed chain {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    sys.exit(rc)
