// quantile.hip — posterior quantiles of a recorded trace on the device (nm_quantile_draws, include/nuts_amd.h): exact order statistics per
// element, pooled over draws and chains, numpy's "linear" positions.  NOT reference behaviour: the definition is this repository's
//  and the header states it operation by operation, so that tests/quantile_ref.py restates it in numpy with the same bits.
//
// A post-pass over buffers the draw calls have written; engine-free like nm_summarize_draws, and no draw kernel is involved.
// The method is a radix selection of ALL requested ranks of ALL columns at once, most significant byte of the 64-bit key first:
//   state          per column: up to R active prefixes (R = the distinct ranks asked for, at most 2 per probability; the prefixes are the
//                  top 8 * pass bits of the keys the ranks lie in, distinct and ascending), per rank the slot of its prefix and the rank
//                  that is left inside that prefix, per (column, slot) a histogram of 256 counts.
//   count kernel   streams the trace once.  A block owns a tile of adjacent columns and a slab of rows; its lanes read contiguous runs
//                  of `row * dim + col` (16 B per lane where the trace allows it), several rows side by side where the tile is narrower
//                  than the block.  An element that carries one of its column's prefixes counts its next byte in the block's LDS
//                  histogram (atomicAdd on uint32_t); the block's non-zero bins are then added to the global histogram (integer atomics).
//   select kernel  one block per column: per slot a scan of the 256 bins; every rank picks the bin it lies in, subtracts the count below
//                  it, the prefix grows by that byte, equal prefixes share one slot again.  It leaves the histogram zeroed.
//   finish kernel  after the eighth byte the prefix IS the key: keys back to doubles, the interpolation, the NaN rule.
// Every number that decides anything is an integer count: the result does not depend on the grid, the block size or arrival order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"

namespace {
constexpr int MAXP = NM_QUANTILE_MAX_PROBS, MAXR = 2 * MAXP;
constexpr int BLOCK = 256, BINS = 256, UNROLL = 4;
constexpr int CBLOCK = 512;           // the count kernel's block: two of them fit a CU's LDS, 16 wavefronts with loads in flight
constexpr int RCAP = 8;               // up to this many prefixes per column live in registers (three probabilities need 6)
constexpr int LDS_SLOTS = 56;          // (column, slot) histograms of 1 KiB a block keeps: 56 KiB + the prefixes, under the 64 KiB of a block

struct Ranks {                          // derived from h_probs on the host; travels in the kernel arguments
    uint32_t rank[MAXR];                // the distinct ranks, ascending
    double g[MAXP];
    uint8_t lo[MAXP], hi[MAXP];         // per probability: index into rank[] (hi == lo when g == 0)
    int n_ranks, n_probs;
};

struct State {                          // device scratch, per column
    uint32_t* hist;                     // [dim][R][256]
    uint64_t* prefix;                   // [dim][R]: the top 8 * pass bits, right-aligned
    uint32_t* slot;                     // [dim][R]: per rank the slot of its prefix
    uint32_t* rem;                      // [dim][R]: per rank what is left of it inside the prefix
    uint32_t* n_prefix;                 // [dim]
    uint32_t* nan;                      // [dim]
};

struct CountArgs {
    const double* x;                    // [N][C][D]
    const uint64_t* ids;                // device, [csel] or null
    State st;
    uint64_t dim, chains, csel, n_rows, rows_per_slab;       // n_rows = N * csel pooled rows
    int R, slots, tile_cols, tile_vecs, groups, pass;          // slots: histograms per column in the block's LDS (1 in the first pass, else R)
};

__device__ inline uint64_t key_of(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull); }
__device__ inline uint64_t bits_of(uint64_t key) { return key ^ ((key >> 63) ? 0x8000000000000000ull : ~0ull); }

__global__ __launch_bounds__(BLOCK) void quantile_init_kernel(State st, Ranks rk, uint64_t dim) {
    const uint64_t d = blockIdx.x;
    const int t = threadIdx.x, R = rk.n_ranks;
    if (d >= dim) return;
    for (int s = 0; s < R; ++s) st.hist[(d * R + s) * BINS + t] = 0;
    if (t < R) {
        st.prefix[d * R + t] = 0;
        st.slot[d * R + t] = 0;
        st.rem[d * R + t] = rk.rank[t];
    }
    if (t == 0) { st.n_prefix[d] = 1; st.nan[d] = 0; }
}

// LDS: bins [tile_cols][slots][256] uint32, prefixes [tile_cols][slots] uint64, n_prefix [tile_cols], nan [tile_cols]
// RC > 0: the thread keeps its columns' prefixes in registers and compares branch-free (a loop over LDS words waits for every one of
// them: 1.85 ms against 0.67 ms of the first pass on K2's trace); RC = 0: more than RCAP prefixes, or the first pass
template <int V, int RC>
__global__ __launch_bounds__(CBLOCK) void quantile_count_kernel(CountArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int t = threadIdx.x, R = A.slots, tc = A.tile_cols;          // R: the LDS stride; global arrays are strided by A.R
    const int n_bins = tc * R * BINS;
    uint32_t* const bins = lds;
    uint64_t* const pref = reinterpret_cast<uint64_t*>(lds + n_bins);          // (n_bins * 4 is a multiple of 1024)
    uint32_t* const npref = reinterpret_cast<uint32_t*>(pref + tc * R);
    uint32_t* const nans = npref + tc;
    const uint64_t col0 = (uint64_t)blockIdx.x * tc;
    for (int i = t; i < n_bins; i += CBLOCK) bins[i] = 0;
    for (int i = t; i < tc * R; i += CBLOCK) {
        const uint64_t col = col0 + i / R;
        pref[i] = col < A.dim ? A.st.prefix[col * A.R + i % R] : 0;
    }
    for (int i = t; i < tc; i += CBLOCK) {
        npref[i] = col0 + i < A.dim ? A.st.n_prefix[col0 + i] : 0;
        nans[i] = 0;
    }
    __syncthreads();
    const int g = t / A.tile_vecs, lc = (t - g * A.tile_vecs) * V;          // row group, first column inside the tile
    const bool col_ok = g < A.groups && col0 + lc < A.dim;                   // (V = 2: dim and tile_cols are even, lc + 1 is in as well)
    const bool first = A.pass == 0;
    const int shift = 56 - 8 * A.pass;
    const uint64_t r0 = (uint64_t)blockIdx.y * A.rows_per_slab;
    const uint64_t r1 = r0 + A.rows_per_slab < A.n_rows ? r0 + A.rows_per_slab : A.n_rows;
    const uint64_t step = (uint64_t)A.groups;
    uint64_t pf[V][RC > 0 ? RC : 1];                       // (no key's top bits are all ones: they are at most 56)
    if constexpr (RC > 0) {
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int s = 0; s < RC; ++s) pf[j][s] = (col_ok && !first && s < (int)npref[lc + j]) ? pref[(lc + j) * R + s] : ~0ull;
    }
    if (col_ok) {
        for (uint64_t r = r0 + g; r < r1; r += step * UNROLL) {
            uint64_t b[UNROLL][V];
            bool ok[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const uint64_t row = r + u * step;
                ok[u] = row < r1;
                uint64_t at = 0;
                if (ok[u]) {
                    if (A.ids) {
                        const uint64_t draw = row / A.csel, cs = row - draw * A.csel;
                        at = (draw * A.chains + A.ids[cs]) * A.dim + col0 + lc;
                    } else {
                        at = row * A.dim + col0 + lc;
                    }
                }
                // (a row past the slab reads the trace's first words instead: always inside the buffer, never counted)
                if constexpr (V == 2) {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(A.x + (ok[u] ? at : 0));
                    b[u][0] = q.x; b[u][1] = q.y;
                } else {
                    b[u][0] = *reinterpret_cast<const uint64_t*>(A.x + (ok[u] ? at : 0));
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (!ok[u]) continue;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int c = lc + j;
                    const uint64_t key = key_of(b[u][j]);
                    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
                    if (first) {
                        if ((b[u][j] & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) atomicAdd(&nans[c], 1u);
                        atomicAdd(&bins[(c * R) * BINS + digit], 1u);
                    } else {
                        const uint64_t top = key >> (shift + 8);
                        if constexpr (RC > 0) {
                            int slot = -1;
#pragma unroll
                            for (int s = 0; s < RC; ++s) slot = pf[j][s] == top ? s : slot;
                            if (slot >= 0) atomicAdd(&bins[(c * R + slot) * BINS + digit], 1u);
                        } else {
                            const int np = (int)npref[c];
                            for (int s = 0; s < np; ++s)
                                if (pref[c * R + s] == top) { atomicAdd(&bins[(c * R + s) * BINS + digit], 1u); break; }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < n_bins; i += CBLOCK) {
        const uint32_t c = bins[i];
        if (c) {
            const int lcol = i / (R * BINS);
            const uint64_t col = col0 + lcol;
            if (col < A.dim) atomicAdd(&A.st.hist[col * A.R * BINS + (i - lcol * R * BINS)], c);
        }
    }
    if (first)
        for (int i = t; i < tc; i += CBLOCK)
            if (nans[i] && col0 + i < A.dim) atomicAdd(&A.st.nan[col0 + i], nans[i]);
}

// one block per column, thread t = bin t
__global__ __launch_bounds__(BLOCK) void quantile_select_kernel(State st, int R, uint64_t dim) {
    __shared__ uint32_t scan[2][BINS];
    __shared__ uint32_t sl[MAXR], rm[MAXR], bin[MAXR], rm_new[MAXR], sl_new[MAXR];
    __shared__ uint64_t pf_new[MAXR];
    const uint64_t d = blockIdx.x;
    const int t = threadIdx.x;
    if (d >= dim) return;
    const int np = (int)st.n_prefix[d];
    if (t < R) { sl[t] = st.slot[d * R + t]; rm[t] = st.rem[d * R + t]; bin[t] = 0; rm_new[t] = 0; }
    __syncthreads();
    for (int s = 0; s < R; ++s) {
        uint32_t* const h = st.hist + (d * R + s) * BINS + t;
        const uint32_t c = s < np ? *h : 0u;
        *h = 0;                                             // the next pass counts from zero
        if (s >= np) continue;                              // (np is the block's: no thread leaves the barriers below alone)
        int cur = 0;
        scan[0][t] = c;
        __syncthreads();
        for (int off = 1; off < BINS; off <<= 1) {
            const uint32_t v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0u);
            scan[cur ^ 1][t] = v;
            cur ^= 1;
            __syncthreads();
        }
        const uint32_t incl = scan[cur][t], excl = incl - c;
        for (int j = 0; j < R; ++j)
            if (sl[j] == (uint32_t)s && c && excl <= rm[j] && rm[j] < incl) { bin[j] = (uint32_t)t; rm_new[j] = rm[j] - excl; }
        __syncthreads();
    }
    if (t == 0) {
        // the ranks ascend, so their prefixes do: equal (slot, bin) pairs are neighbours
        int ns = 0;
        for (int j = 0; j < R; ++j) {
            if (j == 0 || sl[j] != sl[j - 1] || bin[j] != bin[j - 1]) {
                pf_new[ns] = (st.prefix[d * R + sl[j]] << 8) | bin[j];
                ++ns;
            }
            sl_new[j] = (uint32_t)(ns - 1);
        }
        for (int j = 0; j < ns; ++j) st.prefix[d * R + j] = pf_new[j];
        for (int j = 0; j < R; ++j) { st.slot[d * R + j] = sl_new[j]; st.rem[d * R + j] = rm_new[j]; }
        st.n_prefix[d] = (uint32_t)ns;
    }
}

__global__ __launch_bounds__(128) void quantile_finish_kernel(State st, Ranks rk, uint64_t dim, nm_quantile_outputs o) {
    const uint64_t d = (uint64_t)blockIdx.x * 128u + threadIdx.x;
    if (d >= dim) return;
    const int R = rk.n_ranks;
    const uint32_t n_nan = st.nan[d];
    if (o.d_nan_count) static_cast<uint64_t*>(o.d_nan_count)[d] = n_nan;
    if (!o.d_quantiles) return;
    for (int i = 0; i < rk.n_probs; ++i) {
        const uint64_t klo = st.prefix[d * R + st.slot[d * R + rk.lo[i]]], khi = st.prefix[d * R + st.slot[d * R + rk.hi[i]]];
        const double xlo = __longlong_as_double((long long)bits_of(klo)), xhi = __longlong_as_double((long long)bits_of(khi));
        const double gg = rk.g[i];
        double q = xlo;
        if (gg != 0.0 && klo != khi) q = __dadd_rn(xlo, __dmul_rn(gg, __dsub_rn(xhi, xlo)));
        if (n_nan) q = __longlong_as_double(0x7ff8000000000000ll);
        o.d_quantiles[(uint64_t)i * dim + d] = q;
    }
}

thread_local std::string g_qerr;
nm_status qfail(nm_status st, const std::string& msg) { g_qerr = "nm_quantile_draws: " + msg; return st; }
}  // namespace

extern "C" const char* nm_quantile_last_error(void) { return g_qerr.c_str(); }

extern "C" nm_status nm_quantile_draws(const nm_quantile_spec* spec, const double* d_draws, const nm_quantile_outputs* out, void* stream) {
    // ---- everything that can be refused is refused before the first device call
    if (!spec || !d_draws || !out) return qfail(NM_ERR_INVALID_ARG, "null spec, draws or outputs");
    if (!out->d_quantiles && !out->d_nan_count) return qfail(NM_ERR_INVALID_ARG, "both outputs are null");
    const uint64_t N = spec->n_draws, C = spec->n_chains, D = spec->dim;
    if (N == 0 || C == 0 || D == 0) return qfail(NM_ERR_INVALID_ARG, "n_draws, n_chains and dim must be positive");
    if (spec->n_probs < 1 || spec->n_probs > MAXP) return qfail(NM_ERR_INVALID_ARG, "n_probs must be 1 .. 16");
    if (!spec->h_probs) return qfail(NM_ERR_INVALID_ARG, "null h_probs");
    for (uint64_t i = 0; i < spec->n_probs; ++i)
        if (!(spec->h_probs[i] >= 0.0 && spec->h_probs[i] <= 1.0)) return qfail(NM_ERR_INVALID_ARG, "a probability is NaN or outside [0, 1]");
    uint64_t csel = C;
    const uint64_t* h_ids = static_cast<const uint64_t*>(spec->h_chain_ids);
    if (h_ids) {
        csel = spec->n_chain_ids;
        if (csel == 0) return qfail(NM_ERR_INVALID_ARG, "no chain selected");
        for (uint64_t i = 0; i < csel; ++i) {
            if (h_ids[i] >= C) return qfail(NM_ERR_INVALID_ARG, "chain id out of range");
            if (i && h_ids[i] <= h_ids[i - 1]) return qfail(NM_ERR_INVALID_ARG, "chain ids must be strictly increasing");
        }
    }
    if (N > 0xffffffffull / csel) return qfail(NM_ERR_INVALID_ARG, "more than 2^32 - 1 pooled values per element");
    const uint64_t n = N * csel;
    if (D > 0x7fffffffull) return qfail(NM_ERR_INVALID_ARG, "dim above 2^31 - 1");

    // the ranks: h = p (n - 1), lo = floor h, g = h - lo, hi = min(lo + 1, n - 1); hi is a rank of its own only where it is used
    Ranks rk{};
    rk.n_probs = (int)spec->n_probs;
    uint32_t lo[MAXP], hi[MAXP], all[MAXR];
    int n_all = 0;
    for (int i = 0; i < rk.n_probs; ++i) {
        const double h = spec->h_probs[i] * (double)(n - 1), fl = std::floor(h);
        rk.g[i] = h - fl;
        lo[i] = (uint32_t)fl;
        hi[i] = rk.g[i] != 0.0 ? (uint32_t)std::min<uint64_t>((uint64_t)lo[i] + 1, n - 1) : lo[i];
        all[n_all++] = lo[i];
        if (hi[i] != lo[i]) all[n_all++] = hi[i];
    }
    std::sort(all, all + n_all);
    rk.n_ranks = (int)(std::unique(all, all + n_all) - all);
    for (int j = 0; j < rk.n_ranks; ++j) rk.rank[j] = all[j];
    for (int i = 0; i < rk.n_probs; ++i) {
        rk.lo[i] = (uint8_t)(std::lower_bound(all, all + rk.n_ranks, lo[i]) - all);
        rk.hi[i] = (uint8_t)(std::lower_bound(all, all + rk.n_ranks, hi[i]) - all);
    }
    const uint64_t R = (uint64_t)rk.n_ranks;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return qfail(NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    // scratch, 8-byte words first: prefix [D][R], (ids [csel]); then 4-byte words: hist [D][R][256], slot [D][R], rem [D][R], n_prefix [D], nan [D]
    const uint64_t n_ids = h_ids ? csel : 0;
    const uint64_t bytes = (D * R + n_ids) * 8 + (D * R * BINS + 2 * D * R + 2 * D) * 4;
    char* scratch = nullptr;
    hipError_t e = hipMallocAsync((void**)&scratch, bytes, s);
    if (e != hipSuccess) return qfail(NM_ERR_HIP, hipGetErrorString(e));
    State st;
    st.prefix = reinterpret_cast<uint64_t*>(scratch);
    uint64_t* d_ids = n_ids ? st.prefix + D * R : nullptr;
    st.hist = reinterpret_cast<uint32_t*>(st.prefix + D * R + n_ids);
    st.slot = st.hist + D * R * BINS;
    st.rem = st.slot + D * R;
    st.n_prefix = st.rem + D * R;
    st.nan = st.n_prefix + D;
    if (n_ids) {
        e = hipMemcpyAsync(d_ids, h_ids, n_ids * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);          // the caller's array is free on return
        if (e != hipSuccess) { (void)hipFreeAsync(scratch, s); return qfail(NM_ERR_HIP, hipGetErrorString(e)); }
    }
    hipLaunchKernelGGL(quantile_init_kernel, dim3((unsigned)D), dim3(BLOCK), 0, s, st, rk, D);

    CountArgs A;
    A.x = d_draws; A.ids = d_ids; A.st = st; A.dim = D; A.chains = C; A.csel = csel; A.n_rows = n; A.R = (int)R;
    // 16 bytes per lane where every row starts 16-byte aligned
    const bool wide = D % 2 == 0 && (reinterpret_cast<uintptr_t>(d_draws) & 15) == 0;
    for (int pass = 0; pass < 8; ++pass) {
        // the column tile: as many columns as the block's LDS holds histograms for — one slot per column in the first pass, R after it
        const uint64_t slots = pass == 0 ? 1 : R;
        const uint64_t cap = LDS_SLOTS / slots;              // >= 1: R <= 32
        uint64_t tiles = (D + cap - 1) / cap, tc = (D + tiles - 1) / tiles;
        int V = 1;
        if (wide && cap >= 2) { V = 2; tc = tc % 2 == 0 ? tc : tc + 1 <= cap ? tc + 1 : tc - 1; }          // (an even tile: every run starts 16-byte aligned)
        tiles = (D + tc - 1) / tc;
        A.pass = pass;
        A.slots = (int)slots;
        A.tile_cols = (int)tc;
        A.tile_vecs = (int)(tc / V);
        A.groups = CBLOCK / A.tile_vecs;
        // slabs: blocks of at least 2 rounds of loads, about 2048 blocks in all
        const uint64_t per_round = (uint64_t)A.groups * UNROLL;
        uint64_t slabs = (n + 2 * per_round - 1) / (2 * per_round);
        const uint64_t want = tiles >= 2048 ? 1 : 2048 / tiles;
        if (slabs > want) slabs = want;
        if (slabs > 65535) slabs = 65535;
        A.rows_per_slab = (n + slabs - 1) / slabs;
        slabs = (n + A.rows_per_slab - 1) / A.rows_per_slab;
        const size_t lds = (size_t)tc * slots * BINS * 4 + (size_t)tc * slots * 8 + (size_t)tc * 8;
        const dim3 grid((unsigned)tiles, (unsigned)slabs);
        const bool regs = pass > 0 && R <= RCAP;
        if (V == 2 && regs) hipLaunchKernelGGL((quantile_count_kernel<2, RCAP>), grid, dim3(CBLOCK), lds, s, A);
        else if (V == 2) hipLaunchKernelGGL((quantile_count_kernel<2, 0>), grid, dim3(CBLOCK), lds, s, A);
        else if (regs) hipLaunchKernelGGL((quantile_count_kernel<1, RCAP>), grid, dim3(CBLOCK), lds, s, A);
        else hipLaunchKernelGGL((quantile_count_kernel<1, 0>), grid, dim3(CBLOCK), lds, s, A);
        hipLaunchKernelGGL(quantile_select_kernel, dim3((unsigned)D), dim3(BLOCK), 0, s, st, (int)R, D);
    }
    hipLaunchKernelGGL(quantile_finish_kernel, dim3((unsigned)((D + 127) / 128)), dim3(128), 0, s, st, rk, D, *out);
    e = hipGetLastError();
    (void)hipFreeAsync(scratch, s);
    if (e != hipSuccess) return qfail(NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}
