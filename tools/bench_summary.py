"""What nm_summarize_draws costs on the device.  One JSON line per shape:
K2's recorded trace (200 draws x 4096 chains x dim 1024), K4's (100 x 65536 x 10) and 200 x 8192 x 101, max_lag = 32, split on, every
output requested.  Prints milliseconds (median of REPS launches after one warm-up, HIP events on the call's stream), the bytes the
definition reads (2 x trace) over that time, and beside it nm_probe_bandwidth(NM_PROBE_READ) of the same box on an array of the
trace's size (capped at 2 GiB).  `--shape N,C,D` measures one other shape, `--max-lag K` another number of lags."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuts_rs_amd as N  # noqa: E402
from nuts_rs_amd import _lib  # noqa: E402

L = N.load_library()
REPS = 5
MAX_LAG = int(sys.argv[sys.argv.index("--max-lag") + 1]) if "--max-lag" in sys.argv else 32
SHAPES = [("K2 trace", 200, 4096, 1024), ("K4 trace", 100, 65536, 10), ("200 x 8192 x 101", 200, 8192, 101)]
if "--shape" in sys.argv:
    n_, c_, d_ = (int(v) for v in sys.argv[sys.argv.index("--shape") + 1].split(","))
    SHAPES = [("custom", n_, c_, d_)]

for name, n_draws, chains, dim in SHAPES:
    # (filled per draw: a trace of K2's size next to a same-size temporary would not fit every box's free memory)
    x = torch.empty((n_draws, chains, dim), dtype=torch.float64, device="cuda")
    for t in range(n_draws):
        x[t].normal_()
    n, m = n_draws // 2, 2 * chains
    lags = min(MAX_LAG, n - 1)
    shapes = dict(mean=(dim,), sd=(dim,), within_var=(dim,), rhat=(dim,), ess=(dim,), ess_truncated=(dim,), autocorr=(lags + 1, dim),
                  chain_mean=(m, dim), chain_var=(m, dim))
    bufs = {k: torch.empty(s, dtype=torch.int64 if k == "ess_truncated" else torch.float64, device="cuda") for k, s in shapes.items()}
    out = _lib.NmSummaryOutputs()
    for k, b in bufs.items():
        setattr(out, "d_" + k, b.data_ptr())
    spec = _lib.NmSummarySpec(n_draws, chains, dim, 1, MAX_LAG, 0, None)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(REPS + 1):                              # the first launch is the warm-up
        ev[0].record()
        _lib.check_status(L.nm_summarize_draws(C.byref(spec), C.c_void_p(x.data_ptr()), C.byref(out), None), L.nm_summary_last_error)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append(ev[0].elapsed_time(ev[1]))
    t_ms = statistics.median(ms)
    trace_bytes = n_draws * chains * dim * 8
    rhat_max, ess_min = float(bufs["rhat"].max()), float(bufs["ess"].min())
    del x, bufs
    torch.cuda.empty_cache()
    pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
    _lib.check(L.nm_probe_bandwidth(2, min(trace_bytes, 2 << 30), REPS, C.byref(pm), C.byref(br), C.byref(bw)))          # NM_PROBE_READ
    probe = br.value / (pm.value * 1e-3) / 1e9
    rate = 2 * trace_bytes / (t_ms * 1e-3) / 1e9
    print(json.dumps({"shape": name, "n_draws": n_draws, "n_chains": chains, "dim": dim, "max_lag": MAX_LAG, "split": 1, "ms": t_ms, "ms_all": ms,
                      "bytes_read_2x_trace": 2 * trace_bytes, "GBps": rate, "probe_read_GBps": probe, "fraction_of_read_probe": rate / probe,
                      "rhat_max": rhat_max, "ess_min": ess_min, "repeats": REPS}), flush=True)
