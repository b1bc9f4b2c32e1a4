"""What an expanded draw costs on K4 (non-centred 8 schools -> (mu, tau, theta[8])).  One JSON line.
(a) nm_engine_expand on K4's trace shape, 65536 chains x 100 draws x dim 10, as GB/s moved (read + written), next to the copy rate
    nm_probe_bandwidth measures for the same byte count on the same device;
(b) K4's shard (8192 chains, 100 post-warm-up draws) through nm_engine_draw_ex with and without d_expanded: the two interleaved,
    medians of 5 (wall time of the synchronous call)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuts_rs_amd as N  # noqa: E402

L = N.load_library()
REPS = 5

# ---- (a) the expansion alone --------------------------------------------------------------------------------------------------
chains, draws, dim = 65536, 100, 10
rows = chains * draws
b = N.ChainBatch(N.DiagNutsSettings(num_chains=4, seed=1, num_tune=10), N.LogpSpec.eight_schools(), 4)
edim = b.expanded_dim()
pos = torch.randn((rows, dim), dtype=torch.float64, device="cuda")
out = torch.empty((rows, edim), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
stream = torch.cuda.ExternalStream(b.stream())
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ms = []
for i in range(REPS + 1):                              # the first launch is the warm-up
    ev[0].record(stream)
    N._lib.check(L.nm_engine_expand(b._h, rows, C.c_void_p(pos.data_ptr()), C.c_void_p(out.data_ptr())))
    ev[1].record(stream)
    b.synchronize()
    if i:
        ms.append(ev[0].elapsed_time(ev[1]))
expand_ms = statistics.median(ms)
moved = rows * (dim + edim) * 8
pm, br, bw = C.c_double(), C.c_uint64(), C.c_uint64()
N._lib.check(L.nm_probe_bandwidth(0, rows * dim * 8, REPS, C.byref(pm), C.byref(br), C.byref(bw)))       # NM_PROBE_COPY of the same bytes
copy_gbps = (br.value + bw.value) / (pm.value * 1e-3) / 1e9
b.close()

# ---- (b) inside a draw call ---------------------------------------------------------------------------------------------------
chains, draws = 8192, 100
s = N.DiagNutsSettings(num_chains=chains, seed=20260928, num_tune=400)
runs = {}
for name in ("plain", "expanded"):
    e = N.ChainBatch(s, N.LogpSpec.eight_schools(), chains)
    e.set_position(e.init_positions_uniform())
    e.draw_device(400)
    runs[name] = e
d_pos = torch.empty((draws, chains, dim), dtype=torch.float64, device="cuda")
d_ex = torch.empty((draws, chains, edim), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
wall = {"plain": [], "expanded": []}
for i in range(REPS + 1):                              # both engines advance through the same draws; the first round is the warm-up
    for name, e in runs.items():
        t = time.perf_counter()
        e.draw_device_ex(draws, positions=d_pos.data_ptr(), expanded=d_ex.data_ptr() if name == "expanded" else 0)
        if i:
            wall[name].append(time.perf_counter() - t)
for e in runs.values():
    e.close()
plain_ms, expanded_ms = (1e3 * statistics.median(wall[k]) for k in ("plain", "expanded"))
print(json.dumps({
    "expand_rows": rows, "expand_dim": dim, "expand_edim": edim, "expand_ms": expand_ms, "expand_GBps": moved / (expand_ms * 1e-3) / 1e9,
    "probe_copy_GBps_same_bytes": copy_gbps, "expand_over_copy": moved / (expand_ms * 1e-3) / 1e9 / copy_gbps,
    "draw_ex_chains": chains, "draw_ex_draws": draws, "draw_ex_plain_ms": plain_ms, "draw_ex_expanded_ms": expanded_ms,
    "draw_ex_expansion_cost_ms": expanded_ms - plain_ms, "draw_ex_expansion_cost_fraction": expanded_ms / plain_ms - 1.0,
    "repeats": REPS}))
