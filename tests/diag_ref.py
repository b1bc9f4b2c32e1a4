"""The definitions of nm_stats_columns and nm_diagnose_stats (include/nuts_amd.h) restated in numpy WITH THE SAME BITS:
every floating sum serial in the stated order (draws ascending per chain, vectorised over the chains only), every operation one
binary64 + - * /, a row that is not selected selected away (np.where), never multiplied by zero, and every floating result that is a
NaN stored as 0x7FF8000000000000.  A helper of tests/test_diag_cpu.py and tests/test_gpu_diag.py, not a test."""
from dataclasses import dataclass

import numpy as np

from nuts_rs_amd._lib import STATS_DTYPE

STAT_WORDS = 24
CHUNK = 32                                    # NM_SUMMARY_CHUNK_CHAINS
DEPTH_BINS = 32
ALL, SAMPLING, TUNING = 0, 1, 2
UNWRITTEN = np.uint64(2**64 - 1)
NAN_BITS = np.uint64(0x7FF8000000000000)
CHAIN_COUNTS = ("rows", "diverging", "maxdepth", "leapfrogs", "max_depth", "final_status")
CHAIN_VALUES = ("mean_accept", "energy_mean", "energy_var", "bfmi", "mean_logp", "last_step_size")
POOLED_COUNTS = ("healthy", "rows", "diverging", "maxdepth", "leapfrogs", "chains_diverging", "chains_low_bfmi", "chains_nan_bfmi")
POOLED_VALUES = ("mean_accept", "mean_step_size", "min_bfmi")


def canon(x):
    """the array with every NaN replaced by the one NaN the device stores"""
    x = np.array(x, dtype=np.float64)
    b = x.view(np.uint64)
    b[np.isnan(x)] = NAN_BITS
    return x


def field_index(name):
    return list(STATS_DTYPE.names).index(name)


def stats_columns(stats, fields):
    """stats: a STATS_DTYPE array of any shape; fields: names or word indices -> float64 [..., len(fields)]"""
    names = [f if isinstance(f, str) else STATS_DTYPE.names[int(f)] for f in fields]
    out = np.empty(stats.shape + (len(names),), dtype=np.float64)
    unwritten = stats["chain_status"] == UNWRITTEN
    for i, n in enumerate(names):
        col = stats[n]
        out[..., i] = col if col.dtype == np.float64 else col.astype(np.float64)          # a double word: bit for bit
        out[..., i].view(np.uint64)[unwritten] = NAN_BITS
    return out


@dataclass
class Diag:
    chain_counts: np.ndarray             # uint64 [n_chains, 6]
    chain_values: np.ndarray             # float64 [n_chains, 6]
    pooled_counts: np.ndarray            # uint64 [8]
    pooled_values: np.ndarray            # float64 [3]
    depth_hist: np.ndarray               # uint64 [32]
    events: np.ndarray                   # uint64 [min(n_events, max_events), 2]
    n_events: int


def diagnose(stats, phase=ALL, max_events=4096, bfmi_threshold=0.3):
    st = np.ascontiguousarray(stats, dtype=STATS_DTYPE)
    N, C = st.shape
    err = np.seterr(all="ignore")
    try:
        written = st["chain_status"] != UNWRITTEN
        tuning = st["tuning"] != 0
        sel = written & {ALL: np.ones_like(tuning), SAMPLING: ~tuning, TUNING: tuning}[phase]
        z = np.zeros(C)
        k = np.zeros(C, dtype=np.uint64)
        n_div, n_md, leap, maxd = k.copy(), k.copy(), k.copy(), k.copy()
        s_acc, s_e, s_lp, s_d, e_prev = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
        last_step = np.full(C, np.nan)
        for t in range(N):
            s, r = sel[t], st[t]
            e = r["energy"]
            d = e - e_prev
            s_d = np.where(s & (k > 0), s_d + d * d, s_d)
            e_prev = np.where(s, e, e_prev)
            s_e = np.where(s, s_e + e, s_e)
            s_acc = np.where(s, s_acc + r["mean_tree_accept"], s_acc)
            s_lp = np.where(s, s_lp + r["logp"], s_lp)
            last_step = np.where(s, r["step_size"], last_step)
            k = k + s.astype(np.uint64)
            n_div = n_div + (s & (r["diverging"] != 0)).astype(np.uint64)
            n_md = n_md + (s & (r["maxdepth_reached"] != 0)).astype(np.uint64)
            leap = np.where(s, leap + r["n_steps"], leap)                                 # uint64: modulo 2^64
            maxd = np.where(s, np.maximum(maxd, r["depth"]), maxd)
        kd = k.astype(np.float64)
        m = s_e / kd
        s_v = z.copy()
        for t in range(N):
            d = st[t]["energy"] - m
            s_v = np.where(sel[t], s_v + d * d, s_v)
        v = s_v / kd
        bfmi = (s_d / (k - np.uint64(1)).astype(np.float64)) / v                          # k - 1 in uint64 arithmetic
        final = st["chain_status"][N - 1].copy()
        chain_counts = np.stack([k, n_div, n_md, leap, maxd, final], axis=1).astype(np.uint64)
        chain_values = canon(np.stack([s_acc / kd, m, v, bfmi, s_lp / kd, last_step], axis=1))

        healthy = final == 0
        nh = np.uint64(healthy.sum())
        with_nan = np.isnan(bfmi)
        pooled_counts = np.array([nh, k[healthy].sum(dtype=np.uint64), n_div[healthy].sum(dtype=np.uint64), n_md[healthy].sum(dtype=np.uint64),
                                  leap[healthy].sum(dtype=np.uint64), (healthy & (n_div > 0)).sum(), (healthy & (bfmi < bfmi_threshold)).sum(),
                                  (healthy & with_nan).sum()], dtype=np.uint64)

        def pooled_sum(x):
            n_chunks = -(-C // CHUNK)
            pad = n_chunks * CHUNK - C
            xx = np.concatenate([x, np.zeros(pad)]).reshape(n_chunks, CHUNK)
            hh = np.concatenate([healthy, np.zeros(pad, dtype=bool)]).reshape(n_chunks, CHUNK)
            part = np.zeros(n_chunks)
            for j in range(CHUNK):
                part = np.where(hh[:, j], part + xx[:, j], part)
            total = np.float64(0.0)
            for p in part:
                total = total + p
            return total

        fin = healthy & ~with_nan
        pooled_values = canon(np.array([pooled_sum(chain_values[:, 0]) / np.float64(nh), pooled_sum(chain_values[:, 5]) / np.float64(nh),
                                        bfmi[fin].min() if fin.any() else np.inf]))
        rows = sel & healthy[None, :]
        depth_hist = np.bincount(np.minimum(st["depth"][rows], np.uint64(DEPTH_BINS - 1)).astype(np.int64), minlength=DEPTH_BINS).astype(np.uint64)
        ev = np.argwhere(sel & (st["diverging"] != 0)).astype(np.uint64)                  # row-major: lexicographic (t, c)
        return Diag(chain_counts, chain_values, pooled_counts, pooled_values, depth_hist, ev[:max_events].reshape(-1, 2), int(len(ev)))
    finally:
        np.seterr(**err)
