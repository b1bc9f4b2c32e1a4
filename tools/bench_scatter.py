"""What nm_pooled_scatter costs on the device.  One JSON line per shape, all lines also written to profiles/r16_scatter.json:
K5's window (80 draws x 4096 chains x dim 256), K2's (100 x 4096 x 1024) and K4's (100 x 65536 x 10), centred at the rows' mean.
Per shape (a) milliseconds (median of REPS launches after one warm-up, HIP events on the call's stream), 2 n D^2 flop over that time
beside the f64 MFMA rate tools/probes/mfma_f64_rate reports on the same box in the same session (when the probe has been built), the
bytes of the rows once over that time beside nm_probe_bandwidth(NM_PROBE_READ); (b) what a caller could do before on the same device
— Y = X - c; Y.T @ Y in torch f64 — with its time and the memory it allocates beyond the rows.
`--warmup` adds the whole pooled_lowrank_warmup at K5's shape (a correlated normal of dim 256, 4096 chains, num_tune 400) next to the
diagonal pooled_warmup and the kernel time of the window launches it overlaps.  `--shape N,C,D` measures one other shape."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nuts_rs_amd as N  # noqa: E402
from nuts_rs_amd import _lib, pooled  # noqa: E402

L = N.load_library()
REPS = 5
OUT = os.path.join(ROOT, "profiles", "r16_scatter.json")
SHAPES = [("K5 window", 80, 4096, 256), ("K2 window", 100, 4096, 1024), ("K4 window", 100, 65536, 10)]
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


def mfma_rate():
    """(the best TFLOP/s of tools/probes/mfma_f64_rate, its lines as {waves_per_simd, chains_per_wave, TFLOPs}); (None, []) when the probe
    has not been built.  The lines are the measurement of how many independent accumulators a SIMD needs to keep the matrix pipe busy."""
    exe = os.path.join(ROOT, "tools", "probes", "mfma_f64_rate")
    if not os.path.exists(exe):
        return None, []
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    # (a block of the probe is 256 x waves/SIMD threads: its 8 waves/SIMD lines ask for 2048 and never launch)
    lines = [{"waves_per_simd": int(w), "chains_per_wave": int(c), "TFLOPs": float(t)}
             for w, c, t in re.findall(r"waves/SIMD (\d+) chains/wave (\d+):.*? ([0-9.]+) TFLOP/s", r.stdout) if int(w) <= 4]
    return (max(v["TFLOPs"] for v in lines), lines) if r.returncode == 0 and lines else (None, [])


records = []
peak, probe_lines = mfma_rate()
for name, n_draws, chains, dim in SHAPES:
    x = torch.empty((n_draws, chains, dim), dtype=torch.float64, device="cuda")
    for t in range(n_draws):          # (filled per draw: no temporary of the rows' size)
        x[t].normal_()
    n = n_draws * chains
    rows = x.view(n, dim)
    c = rows.mean(dim=0)
    S = torch.empty((dim, dim), dtype=torch.float64, device="cuda")
    cnt = torch.empty((1,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def ours():
        _lib.check_status(L.nm_pooled_scatter(n, dim, x.data_ptr(), c.data_ptr(), None, S.data_ptr(), cnt.data_ptr(), None), L.nm_pooled_last_error)

    t_ms, ms, _ = timed(ours)
    row_bytes = n * dim * 8
    tiles = -(-dim // 64)
    n_slabs = min(max(-(-n // N.NM_SCATTER_SLAB_MIN_ROWS), 1), N.NM_SCATTER_MAX_SLABS)
    rec = {"shape": name, "n_draws": n_draws, "n_chains": chains, "dim": dim, "ms": t_ms, "ms_all": ms, "repeats": REPS,
           "flop_2nD2": 2.0 * n * dim * dim, "TFLOPs": 2.0 * n * dim * dim / (t_ms * 1e-3) / 1e12, "mfma_f64_probe_TFLOPs": peak,
           "row_bytes": row_bytes, "rows_once_GBps": row_bytes / (t_ms * 1e-3) / 1e9, "row_reads": tiles,
           "rows_as_read_GBps": tiles * row_bytes / (t_ms * 1e-3) / 1e9,
           "scratch_bytes": (n_slabs * (tiles * (tiles + 1) // 2) * 4096 + n_slabs) * 8, "count": float(cnt.item())}
    rec["executed_TFLOPs"] = rec["TFLOPs"] * (tiles + 1) / (2 * tiles)          # the upper-triangle tiles only: T (T + 1) / 2 of T^2
    if peak:
        rec["executed_fraction_of_mfma_probe"] = rec["executed_TFLOPs"] / peak

    def by_torch():
        y = rows - c
        return y.T @ y

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    try:
        m_ms, m_all, ref = timed(by_torch)
        extra = torch.cuda.max_memory_allocated() - before
        scale = torch.sqrt(torch.outer(torch.diagonal(ref), torch.diagonal(ref)))
        rec.update({"torch_ms": m_ms, "torch_ms_all": m_all, "torch_extra_bytes": int(extra), "torch_over_ours": m_ms / t_ms,
                    "max_difference_in_units_of_sqrt_Sii_Sjj": float(((ref - S).abs() / scale).max())})
        del ref, scale
    except torch.cuda.OutOfMemoryError as e:          # the rows' size again does not fit beside them
        rec["torch_error"] = str(e)[:200]
    del x, rows
    torch.cuda.empty_cache()
    pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
    _lib.check(L.nm_probe_bandwidth(2, min(row_bytes, 2 << 30), REPS, C.byref(pm), C.byref(br), C.byref(bw)))          # NM_PROBE_READ
    probe = br.value / (pm.value * 1e-3) / 1e9
    rec.update({"probe_read_GBps": probe, "rows_once_fraction_of_read_probe": rec["rows_once_GBps"] / probe,
                "rows_as_read_fraction_of_read_probe": rec["rows_as_read_GBps"] / probe})
    records.append(rec)
    print(json.dumps(rec), flush=True)

if "--warmup" in sys.argv:
    dim, chains, tune = 256, 4096, 400
    rng = np.random.default_rng(5)
    u = np.linalg.qr(rng.normal(size=(dim, 16)))[0]
    sigma = np.eye(dim) + u @ np.diag(rng.uniform(5.0, 50.0, 16)) @ u.T
    sc = np.exp(rng.normal(0, 0.5, dim))
    sigma = np.diag(sc) @ sigma @ np.diag(sc)
    prec = np.linalg.inv(sigma)
    prec = (prec + prec.T) / 2
    for which in ("pooled_lowrank_warmup", "pooled_warmup"):
        s = N.LowRankNutsSettings(num_chains=chains, seed=3, num_tune=tune, freeze_transform=True)
        b = N.ChainBatch(s, N.LogpSpec.mvn_precision(prec), chains)
        assert (b.set_position(b.init_positions_uniform()) == 0).all()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ups = getattr(pooled, which)(b, tune)
        b.synchronize()
        wall = time.perf_counter() - t0
        counters = b.counters()
        pos, st = b.draw_many(100)
        rec = {"shape": "K5 warm-up", "driver": which, "dim": dim, "n_chains": chains, "num_tune": tune, "windows": pooled.window_schedule(tune),
               "wall_s": wall, "window_kernel_ms": counters["kernel_ms"], "updates": len(ups), "rank_of_last_update": int(len(ups[-1][3])) if which == "pooled_lowrank_warmup" and ups else 0,
               "tile_launches": b.tile_launches(), "lockstep_launches": b.lockstep_launches(),
               "leapfrogs_per_draw_after": float(st["n_steps"].mean())}
        b.close()
        records.append(rec)
        print(json.dumps(rec), flush=True)

if "--shape" not in sys.argv:
    with open(OUT, "w") as f:
        json.dump({"tool": "tools/bench_scatter.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0), "mfma_f64_probe": probe_lines,
                   "records": records}, f, indent=1)
