"""What nm_transform_draws and rank_diagnostics cost on the device.  One JSON record per shape: K4's recorded trace
(100 draws x 65536 chains x dim 10) and K2's (100 x 4096 x 1024).  Per shape (a) kind 0 (the normal scores of the pooled ranks, scores
and NaN counts requested): milliseconds (median of REPS launches after one warm-up, HIP events on the call's stream), the bytes the
method moves over that time — per key the gather reads 8 and writes 12, each of the 8 passes reads 8 (count) + 12 and writes 12
(scatter), the score kernel reads 12 and writes 8: 296 in all —, the scratch of the call; (b) the whole rank_diagnostics (wall clock
around the Python call, device synchronised; it contains seven device calls and their host round trips); (c) what a caller can do today
on the same device in the same process — torch.sort along the pooled axis with its indices, the scores of the positions by
torch.special.ndtri, a scatter of them to the elements' places — with its time and the memory it allocates beyond the trace and the
output; (d) nm_probe_bandwidth(NM_PROBE_READ) of the same box on an array of the trace's size (capped at 2 GiB).
Writes the records to profiles/ under the next free number (`--out PATH`: elsewhere) and prints them.
`--shape N,C,D` measures one other shape, `--no-sort` leaves (c) out, `--no-diagnostics` leaves (b) out (the run a kernel trace is
taken from), `--max-scratch BYTES` bounds the call's scratch."""
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nuts_rs_amd as N  # noqa: E402
from nuts_rs_amd import _lib  # noqa: E402

L = N.load_library()
REPS = 5
BYTES_PER_KEY = 20 + 8 * 32 + 20
SHAPES = [("K4 trace", 100, 65536, 10), ("K2 trace", 100, 4096, 1024)]
if "--shape" in sys.argv:
    n_, c_, d_ = (int(v) for v in sys.argv[sys.argv.index("--shape") + 1].split(","))
    SHAPES = [("custom", n_, c_, d_)]
MAX_SCRATCH = int(sys.argv[sys.argv.index("--max-scratch") + 1]) if "--max-scratch" in sys.argv else 0


def next_profile_path():
    numbers = [int(m.group(1)) for m in (re.match(r"r(\d+)", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(numbers, default=0) + 1}_rank_transform.json")


def timed(fn, wall=False):
    """median milliseconds of REPS calls after one warm-up, and the last result"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms, res = [], None
    for i in range(REPS + 1):
        res = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        res = fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3 if wall else ev[0].elapsed_time(ev[1]))
    return statistics.median(ms), ms, res


records = []
for name, n_draws, chains, dim in SHAPES:
    # (filled per draw: a trace of K2's size next to a same-size temporary would not fit every box's free memory)
    x = torch.empty((n_draws, chains, dim), dtype=torch.float64, device="cuda")
    for t in range(n_draws):
        x[t].normal_()
    n = n_draws * chains
    out = torch.empty((n_draws, chains, dim), dtype=torch.float64, device="cuda")
    nan = torch.empty((dim,), dtype=torch.int64, device="cuda")
    o = _lib.NmTransformOutputs(out.data_ptr(), None, nan.data_ptr())
    spec = _lib.NmTransformSpec(n_draws, chains, dim, N.NM_TRANSFORM_RANK_NORMAL, 1, 0, None, MAX_SCRATCH)
    torch.cuda.synchronize()

    def ours():
        _lib.check_status(L.nm_transform_draws(C.byref(spec), C.c_void_p(x.data_ptr()), None, C.byref(o), None), L.nm_transform_last_error)

    t_ms, ms, _ = timed(ours)
    slabs = -(-n // N.NM_RANK_SLAB_KEYS)
    per_col = 24 * n + 1024 * slabs
    cols = max(1, min(dim, 32768, (MAX_SCRATCH or 1 << 30) // per_col))
    if dim % 2 == 0 and cols > 1 and cols % 2:
        cols -= 1
    trace_bytes = n * dim * 8
    rec = {"shape": name, "n_draws": n_draws, "n_chains": chains, "dim": dim, "kind": 0, "ms": t_ms, "ms_all": ms,
           "bytes_moved_296_per_key": BYTES_PER_KEY * n * dim, "GBps": BYTES_PER_KEY * n * dim / (t_ms * 1e-3) / 1e9,
           "scratch_bytes": cols * per_col + 4 * dim, "columns_per_batch": cols, "batches": -(-dim // cols), "trace_bytes": trace_bytes,
           "nan_total": int(nan.sum().item()), "repeats": REPS}

    if "--no-diagnostics" not in sys.argv:
        d_ms, d_all, rd = timed(lambda: N.rank_diagnostics(x, split=True, max_lag=32, max_scratch_bytes=MAX_SCRATCH), wall=True)
        rec.update({"rank_diagnostics_wall_ms": d_ms, "rank_diagnostics_wall_ms_all": d_all, "rhat_rank_max": float(rd.rhat_rank.max()),
                    "ess_bulk_min_over_n": float(rd.ess_bulk.min() / n), "ess_tail_min_over_n": float(rd.ess_tail.min() / n)})

    if "--no-sort" not in sys.argv:
        ours()
        torch.cuda.synchronize()
        pos = (torch.arange(1, n + 1, dtype=torch.float64, device="cuda") - 0.375) / (n + 0.25)
        scores_by_position = torch.special.ndtri(pos)[:, None].expand(n, dim)
        ref = torch.empty((n, dim), dtype=torch.float64, device="cuda")

        def by_sort():
            idx = x.view(n, dim).sort(dim=0).indices
            ref.scatter_(0, idx, scores_by_position)

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        s_ms, s_all, _ = timed(by_sort)
        extra = torch.cuda.max_memory_allocated() - before
        diff = float((ref - out.view(n, dim)).abs().max().item())          # (tie-free data: ordinal ranks are average ranks)
        rec.update({"sort_ms": s_ms, "sort_ms_all": s_all, "sort_extra_bytes": int(extra), "speedup_over_sort": s_ms / t_ms,
                    "scratch_fraction_of_sort": rec["scratch_bytes"] / max(1, int(extra)), "max_abs_diff_to_sort_route": diff})
        del ref, scores_by_position, pos
    del x, out
    torch.cuda.empty_cache()
    pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
    _lib.check(L.nm_probe_bandwidth(2, min(trace_bytes, 2 << 30), REPS, C.byref(pm), C.byref(br), C.byref(bw)))          # NM_PROBE_READ
    probe = br.value / (pm.value * 1e-3) / 1e9
    rec.update({"probe_read_GBps": probe, "fraction_of_read_probe": rec["GBps"] / probe})
    print(json.dumps(rec), flush=True)
    records.append(rec)

path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else next_profile_path()
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump({"what": "tools/bench_rank.py on one device: see its docstring", "argv": sys.argv[1:], "bench_rank": records}, f, indent=1)
print("wrote", path)
