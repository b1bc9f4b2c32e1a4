"""What nm_quantile_draws costs on the device.  One JSON line per shape:
K4's recorded trace (100 draws x 65536 chains x dim 10) and K2's (100 x 4096 x 1024), probabilities 0.05 / 0.5 / 0.95, both outputs
requested.  Prints (a) milliseconds (median of REPS launches after one warm-up, HIP events on the call's stream), the bytes the method
reads (8 passes x trace) over that time, and beside it nm_probe_bandwidth(NM_PROBE_READ) of the same box on an array of the trace's
size (capped at 2 GiB); (b) what a caller could do before on the same device — torch.sort along the pooled axis plus two gathers and
the interpolation — with its time and the memory it allocates beyond the trace, next to the scratch of the new call.
`--shape N,C,D` measures one other shape, `--probs a,b,c` other probabilities, `--no-sort` leaves (b) out."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuts_rs_amd as N  # noqa: E402
from nuts_rs_amd import _lib  # noqa: E402

L = N.load_library()
REPS = 5
PASSES = 8
PROBS = [float(v) for v in sys.argv[sys.argv.index("--probs") + 1].split(",")] if "--probs" in sys.argv else [0.05, 0.5, 0.95]
SHAPES = [("K4 trace", 100, 65536, 10), ("K2 trace", 100, 4096, 1024)]
if "--shape" in sys.argv:
    n_, c_, d_ = (int(v) for v in sys.argv[sys.argv.index("--shape") + 1].split(","))
    SHAPES = [("custom", n_, c_, d_)]


def timed(fn):
    """median milliseconds of REPS calls after one warm-up, and the last result"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms, res = [], None
    for i in range(REPS + 1):
        res = None
        ev[0].record()
        res = fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms), ms, res


for name, n_draws, chains, dim in SHAPES:
    # (filled per draw: a trace of K2's size next to a same-size temporary would not fit every box's free memory)
    x = torch.empty((n_draws, chains, dim), dtype=torch.float64, device="cuda")
    for t in range(n_draws):
        x[t].normal_()
    n = n_draws * chains
    p = np.ascontiguousarray(PROBS, dtype=np.float64)
    q = torch.empty((len(p), dim), dtype=torch.float64, device="cuda")
    nan = torch.empty((dim,), dtype=torch.int64, device="cuda")
    out = _lib.NmQuantileOutputs(q.data_ptr(), nan.data_ptr())
    spec = _lib.NmQuantileSpec(n_draws, chains, dim, len(p), p.ctypes.data, 0, None)
    torch.cuda.synchronize()

    def ours():
        _lib.check_status(L.nm_quantile_draws(C.byref(spec), C.c_void_p(x.data_ptr()), C.byref(out), None), L.nm_quantile_last_error)

    t_ms, ms, _ = timed(ours)
    trace_bytes = n * dim * 8
    h = p * np.float64(n - 1)
    lo = np.floor(h)
    g = h - lo
    n_ranks = len(set(lo.astype(np.int64).tolist()) | set((lo + 1).astype(np.int64)[g != 0].tolist()))
    scratch = dim * n_ranks * 1040 + dim * 8
    rec = {"shape": name, "n_draws": n_draws, "n_chains": chains, "dim": dim, "probs": PROBS, "passes": PASSES, "ms": t_ms, "ms_all": ms,
           "bytes_read_8x_trace": PASSES * trace_bytes, "GBps": PASSES * trace_bytes / (t_ms * 1e-3) / 1e9, "scratch_bytes": scratch,
           "repeats": REPS}

    if "--no-sort" not in sys.argv:
        lo_t = torch.from_numpy(lo.astype(np.int64)).cuda()
        hi_t = torch.clamp(lo_t + 1, max=n - 1)
        g_t = torch.from_numpy(g).cuda()[:, None]

        def by_sort():
            v = x.view(n, dim).sort(dim=0).values
            a, b = v[lo_t], v[hi_t]
            return a + g_t * (b - a)

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        s_ms, s_all, ref = timed(by_sort)
        extra = torch.cuda.max_memory_allocated() - before
        same = bool(((ref == q) | (ref.isnan() & q.isnan())).all())
        rec.update({"sort_ms": s_ms, "sort_ms_all": s_all, "sort_extra_bytes": int(extra), "speedup_over_sort": s_ms / t_ms,
                    "scratch_fraction_of_sort": scratch / max(1, int(extra)), "equals_sort_result": same})
        del ref
    del x
    torch.cuda.empty_cache()
    pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
    _lib.check(L.nm_probe_bandwidth(2, min(trace_bytes, 2 << 30), REPS, C.byref(pm), C.byref(br), C.byref(bw)))          # NM_PROBE_READ
    probe = br.value / (pm.value * 1e-3) / 1e9
    rec.update({"probe_read_GBps": probe, "fraction_of_read_probe": rec["GBps"] / probe})
    print(json.dumps(rec), flush=True)
