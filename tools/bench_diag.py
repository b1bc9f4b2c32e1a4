"""What nm_diagnose_stats and nm_stats_columns cost on the device, next to the route without them.  One JSON record per
shape: 400 draws x 65536 chains (K4's many-chain run) and 1000 x 4096.  Per shape (a) nm_diagnose_stats with every output (phase
"sampling", 4096 events): milliseconds (median of REPS launches after one warm-up, HIP events around the call) and the rate at which
that reads the records (192 bytes each; the energy scratch, 8 bytes written and read per selected row, is not counted), which of the
two alignment paths ran and the energy strategy; (b) nm_stats_columns with 2 fields, the same way; (c) nm_probe_bandwidth(NM_PROBE_READ)
of the same box on an array of the records' size (capped at 2 GiB) and the fraction of it each rate is; (d) the route the library
offered before: the copy of the whole record array to the host — `tensor.cpu()` as ChainBatch.draw_summary does it, and into pinned
memory, the best a PCIe copy can do — and the numpy restatement tests/diag_ref.py over that copy, wall clock.
Writes the records to profiles/ under the next free number (`--out PATH`: elsewhere) and prints them.  `--shape N,C` measures one other
shape, `--no-host` leaves (d)'s restatement out (the copies stay: they are the pass condition).  The energy strategy of §31 was chosen with
this tool: `python tools/build_variant.py reread "-DNM_DIAG_REREAD_ENERGY=1" stats_diag.hip` builds the variant that walks the records a
second time instead of spilling the energies; run it with NUTS_AMD_LIB=<that library> and `--energy-strategy reread` (the label recorded)."""
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nuts_rs_amd as N  # noqa: E402
from nuts_rs_amd import _lib  # noqa: E402

L = N.load_library()
REPS = 5
MAX_EVENTS = 4096
ITEM = N.STATS_DTYPE.itemsize
WORD = {name: i for i, name in enumerate(N.STATS_DTYPE.names)}
SHAPES = [("K4 many-chain run", 400, 65536), ("1000 x 4096", 1000, 4096)]
STRATEGIES = {"spill": "spilled to [n_draws][n_chains] scratch in the first pass, read back by the same lane",
              "reread": "no scratch: the records are walked a second time (the -DNM_DIAG_REREAD_ENERGY=1 measurement build)"}
STRATEGY = STRATEGIES[sys.argv[sys.argv.index("--energy-strategy") + 1] if "--energy-strategy" in sys.argv else "spill"]
if "--shape" in sys.argv:
    n_, c_ = (int(v) for v in sys.argv[sys.argv.index("--shape") + 1].split(","))
    SHAPES = [("custom", n_, c_)]


def next_profile_path():
    numbers = [int(m.group(1)) for m in (re.match(r"r(\d+)", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(numbers, default=0) + 1}_stats_diag.json")


def timed(fn, wall=False, reps=REPS):
    """median milliseconds of `reps` calls after one warm-up"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3 if wall else ev[0].elapsed_time(ev[1]))
    return statistics.median(ms), ms


def synthetic_records(n_draws, chains):
    """plausible records built on the device, a draw at a time: a tenth of the rows tuning, 1 % divergent, depths 1 .. 10"""
    words = torch.zeros((n_draws, chains, ITEM // 8), dtype=torch.int64, device="cuda")
    reals = words.view(torch.float64)
    chain = torch.arange(chains, dtype=torch.int64, device="cuda")
    for t in range(n_draws):
        words[t, :, WORD["draw"]], words[t, :, WORD["chain"]] = t, chain
        depth = torch.randint(1, 11, (chains,), device="cuda")
        words[t, :, WORD["depth"]], words[t, :, WORD["n_steps"]] = depth, 2 ** depth - 1
        words[t, :, WORD["maxdepth_reached"]] = (depth == 10).long()
        words[t, :, WORD["diverging"]] = (torch.rand(chains, device="cuda") < 0.01).long()
        words[t, :, WORD["tuning"]] = int(t < n_draws // 10)
        for name in ("step_size", "step_size_bar", "mean_tree_accept", "mean_tree_accept_sym"):
            reals[t, :, WORD[name]] = torch.rand(chains, dtype=torch.float64, device="cuda")
        for name in ("logp", "energy", "energy_error", "max_energy_error", "fisher_distance"):
            reals[t, :, WORD[name]] = torch.randn(chains, dtype=torch.float64, device="cuda")
        for name in ("divergence_energy_error", "energy_change", "average_step_size"):
            reals[t, :, WORD[name]] = float("nan")
    return words.view(torch.uint8)


records = []
for name, n_draws, chains in SHAPES:
    st = synthetic_records(n_draws, chains)
    n_rows, nbytes = n_draws * chains, n_draws * chains * ITEM
    bufs = [torch.empty(s, dtype=d, device="cuda") for s, d in (((chains, 6), torch.int64), ((chains, 6), torch.float64), ((8,), torch.int64), ((3,), torch.float64),
                                                                ((32,), torch.int64), ((MAX_EVENTS, 2), torch.int64), ((1,), torch.int64))]
    out = _lib.NmDiagOutputs(*(b.data_ptr() for b in bufs))
    spec = _lib.NmDiagSpec(n_draws, chains, _lib.NM_DIAG_SAMPLING, MAX_EVENTS, 0.3)
    fields = np.array([WORD["energy"], WORD["logp"]], dtype=np.uint64)
    cols = torch.empty((n_draws, chains, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def diagnose():
        _lib.check_status(L.nm_diagnose_stats(C.byref(spec), C.c_void_p(st.data_ptr()), C.byref(out), None), L.nm_diag_last_error)

    def columns():
        _lib.check_status(L.nm_stats_columns(n_rows, 2, fields.ctypes.data, C.c_void_p(st.data_ptr()), C.c_void_p(cols.data_ptr()), None), L.nm_diag_last_error)

    d_ms, d_all = timed(diagnose)
    c_ms, c_all = timed(columns)
    rec = {"shape": name, "n_draws": n_draws, "n_chains": chains, "record_bytes": nbytes, "alignment_path": "16-byte" if st.data_ptr() % 16 == 0 else "8-byte",
           "energy_strategy": STRATEGY, "library": os.path.basename(_lib.LIB_PATH),
           "diagnose_ms": d_ms, "diagnose_ms_all": d_all, "diagnose_read_GBps": nbytes / (d_ms * 1e-3) / 1e9,
           "columns2_ms": c_ms, "columns2_ms_all": c_all, "columns2_read_GBps": nbytes / (c_ms * 1e-3) / 1e9,
           "n_events": int(bufs[6].item()), "pooled_counts": bufs[2].tolist(), "repeats": REPS}

    host = {}

    def copy_pageable():
        host["st"] = st.cpu()

    pinned = torch.empty((n_draws, chains, ITEM), dtype=torch.uint8, pin_memory=True)
    p_ms, p_all = timed(copy_pageable, wall=True, reps=3)
    q_ms, q_all = timed(lambda: pinned.copy_(st, non_blocking=True), wall=True, reps=3)
    rec.update({"d2h_cpu_ms": p_ms, "d2h_cpu_ms_all": p_all, "d2h_pinned_ms": q_ms, "d2h_pinned_ms_all": q_all,
                "d2h_pinned_GBps": nbytes / (q_ms * 1e-3) / 1e9,
                "diagnose_speedup_over_fastest_copy": min(p_ms, q_ms) / d_ms, "columns2_speedup_over_fastest_copy": min(p_ms, q_ms) / c_ms,
                "device_route_faster_than_copy_alone": bool(d_ms < min(p_ms, q_ms) and c_ms < min(p_ms, q_ms))})
    if "--no-host" not in sys.argv:
        import diag_ref
        arr = host["st"].numpy().view(N.STATS_DTYPE).reshape(n_draws, chains)
        t0 = time.perf_counter()
        want = diag_ref.diagnose(arr, diag_ref.SAMPLING, MAX_EVENTS, 0.3)
        rec["host_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        rec["host_route_ms"] = p_ms + rec["host_restatement_ms"]
        rec["equals_host_restatement"] = bool((bufs[0].cpu().numpy().view(np.uint64) == want.chain_counts).all()
                                              and (bufs[1].cpu().numpy().view(np.uint64) == want.chain_values.view(np.uint64)).all()
                                              and (bufs[2].cpu().numpy().view(np.uint64) == want.pooled_counts).all()
                                              and (bufs[3].cpu().numpy().view(np.uint64) == want.pooled_values.view(np.uint64)).all()
                                              and int(bufs[6].item()) == want.n_events
                                              and (bufs[5].cpu().numpy().view(np.uint64)[:min(want.n_events, MAX_EVENTS)] == want.events).all())
    del st, cols, pinned, host
    torch.cuda.empty_cache()
    pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
    _lib.check(L.nm_probe_bandwidth(2, min(nbytes, 2 << 30), REPS, C.byref(pm), C.byref(br), C.byref(bw)))          # NM_PROBE_READ
    probe = br.value / (pm.value * 1e-3) / 1e9
    rec.update({"probe_read_GBps": probe, "diagnose_fraction_of_read_probe": rec["diagnose_read_GBps"] / probe,
                "columns2_fraction_of_read_probe": rec["columns2_read_GBps"] / probe})
    print(json.dumps(rec), flush=True)
    records.append(rec)

path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else next_profile_path()
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump({"what": "tools/bench_diag.py on one device: see its docstring", "argv": sys.argv[1:], "bench_diag": records}, f, indent=1)
print("wrote", path)
