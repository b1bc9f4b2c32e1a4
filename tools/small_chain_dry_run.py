"""Oracle-only dry run (no GPU) of the case lists of tests/test_gpu_small_chain_instantiations.py, of
`test_instantiation_bit_exact_generic_inputs` (tests/test_gpu_every_instantiation.py) and of tests/test_gpu_host_callback_instantiations.py:
those tests skip nothing, so every case must be one in which the oracle accepts every initial point and no sampled chain fails.  A case
reported here gets another seed in the test file's SEEDS / GENERIC_SEEDS / TAX_SEEDS.

The host-callback pass also reports a case whose trees stay below depth 3, an error-taxonomy case whose wall or fatal region is never met
(or in which no chain is left to go on), and prints the oracle's wall time of every case.

The vector-output pass (tests/test_gpu_vector_outputs.py) checks that every case's seed makes the events happen that the case is about, and
looks for a seed where it does not.

    python tools/small_chain_dry_run.py [--cus 256] [--only small|generic|hostcb|vectors]"""
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


def hostcb():
    import test_gpu_host_callback_instantiations as H
    from helpers import estimator_pair
    from nuts_rs_amd import selftest_cases as SC
    bad, cases = [], H.hostcb_cases()
    for c in cases:
        cid = SC.case_id(c)
        if H.tiling_id(c) in H.REFUSED:
            print(f"  {cid}: refused by the engine's plan ({H.REFUSED[H.tiling_id(c)]})")
            continue
        s, draws, adapting = H.make_run(c)
        x0 = O.init_positions_uniform(s.seed, 0, H.N_CHAINS, c["dim"])
        est = estimator_pair(O)[0] if adapting else None
        pos, st, failed, secs = H.oracle_side(O, c, s, draws, x0, 64 * c["w"], 0, est)
        why = []
        if failed or not (st["chain_status"] == 0).all() or not np.isfinite(pos).all():
            why.append(f"chains {failed} rejected their initial point or failed")
        elif st["depth"].max() < 3:
            why.append(f"depth.max() = {int(st['depth'].max())} < 3")
        print(f"  {cid}: {secs:.2f} s, {int(st['n_steps'].sum())} leapfrogs, depth <= {int(st['depth'].max())}, {int(st['diverging'].sum())} divergent draws"
              + "".join("  <-- " + w for w in why))
        if why:
            bad.append(cid)
    tax = H.taxonomy_cases()
    for c in tax:
        t = time.time()
        res = H.taxonomy_oracle(O, c)
        why = H.taxonomy_findings(c, res)
        stopped = {k: len(rows) - 1 for k, (rc, rows) in enumerate(res) if rows and rows[-1][2] != 0}
        nan_div = sum(1 for rc, rows in res for (_, q, rc2) in rows if rc2 == 0 and q["diverging"] and np.isnan(q["divergence_energy_error"]))
        print(f"  {H.taxonomy_id(c)}: {time.time() - t:.2f} s, {nan_div} divergent draws without an energy error, chains stopped (chain: draw) {stopped}"
              + "".join("  <-- " + w for w in why))
        if why:
            bad.append(H.taxonomy_id(c))
    return len(cases), len(tax), bad


def vectors():
    """tests/test_gpu_vector_outputs.py: every case's oracle side with its committed seed must meet the case's conditions (a divergent leapfrog
    from the initial point and one from elsewhere, a mass-matrix event after draw 0, a draw that stays and one that moves, both sides of the
    end of tuning — less what the case drops by construction).  A case that does not is reported; its seeds 0 .. 31 are then run and the
    first that does is printed (for the test file's SEEDS), or that there is none."""
    import test_gpu_vector_outputs as V
    bad, cases = [], V.all_cases()
    for c in cases:
        t = time.time()
        first, why = None, []
        for seed in ([c["seed"]] + [s for s in range(32) if s != c["seed"]]):
            cc = dict(c, seed=seed)
            o = V.oracle_side(O, cc)
            why_s = (["an oracle chain failed"] if o["failed"] else []) + V.findings(cc, o["x0"], o["pos"], o["st"], o["vec"])
            if seed == c["seed"]:
                why = why_s
                e = V.events(cc, o["x0"], o["pos"], o["st"], o["vec"])
                note = (f"{int(e['div'].sum())} divergent draws ({int(e['div0'].sum())} from the initial point), {int(e['upd'][1:].sum())} mass-matrix events after "
                        f"draw 0, {int(e['stay'].sum())} draws stay, {int(o['st']['n_steps'].sum())} leapfrogs, depth <= {int(o['st']['depth'].max())}")
            if not why_s:
                first = seed
                break
        print(f"  {c['id']} (seed {c['seed']}): {time.time() - t:.2f} s, {note}" + "".join("  <-- " + w for w in why)
              + (f"  [first seed of 0 .. 31 that meets the conditions: {first}]" if why else ""))
        if why:
            bad.append(c["id"])
    return len(cases), bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--only", choices=["small", "generic", "hostcb", "vectors"])
    a = ap.parse_args()
    O.lib()
    rc = 0
    if a.only in (None, "small"):
        t = time.time()
        n, chains, div, bad = small(a.cus)
        print(f"small-chain matrix: {n} cases, {chains} oracle chains, {div} divergent draws, {len(bad)} cases with a failed chain {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    if a.only in (None, "generic"):
        t = time.time()
        n, chains, bad = generic()
        print(f"generic inputs: {n} cases, {chains} oracle chains, {len(bad)} cases with a failed chain {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    if a.only in (None, "hostcb"):
        t = time.time()
        n, n_tax, bad = hostcb()
        print(f"host-callback instantiations: {n} cases + {n_tax} error-taxonomy cases, {len(bad)} cases reported {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    if a.only in (None, "vectors"):
        t = time.time()
        n, bad = vectors()
        print(f"vector outputs: {n} cases, {len(bad)} cases reported {bad}, {time.time() - t:.1f} s")
        rc |= bool(bad)
    sys.exit(rc)
