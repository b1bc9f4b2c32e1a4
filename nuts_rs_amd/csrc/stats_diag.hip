// stats_diag.hip — sampler diagnostics from the recorded draw statistics, on the device (nm_stats_columns, nm_diagnose_stats:
// include/nuts_amd.h).  NOT reference behaviour: the definitions are this repository's, the header states them,
// tests/diag_ref.py restates them in numpy with the same bits.
//
// Post-passes over a buffer the draw calls have written; engine-free, no draw kernel is involved.  The records are an array of
// structures with a stride of NM_STAT_WORDS words; the 64 records of (one draw, 64 consecutive chains) are one contiguous run.  Every
// kernel that reads records stages such a run into LDS with the whole block (16 B per lane where the base allows it, 8 B otherwise:
// the stride is a multiple of 16, so the base decides for every run) and lets the lanes pick their words from LDS, one record per
// lane, records one word apart in the banks (a padded stride of NM_STAT_WORDS + 1 words).
//   columns kernel   a block walks runs of 64 records and writes the chosen words, converted, as one contiguous piece of d_out.
//   chain kernel     a block owns 64 consecutive chains and walks the draws in order, G runs at a time: while wavefront 0 adds up the G
//                    staged draws — a lane is a chain, so every floating sum is serial in t — the loads of the next G are in flight.
//                    The energies of the selected rows go to scratch [k][chain]; the same lane reads them back for the centred sum.
//                    The divergent lanes of a (draw, 64 chains) run are one 64-bit mask (__ballot) in a table [draw][group].
//   pool kernels     the two floating means over the healthy chains: a thread per chunk of NM_SUMMARY_CHUNK_CHAINS chains, then one
//                    thread per quantity over the chunk partials in chunk order.  Integer sums arrive by atomics (order-free).
//   event kernels    a STABLE compaction of the mask table, which lies in (t, group) order: bit counts per block of 1024 masks, an
//                    exclusive scan of those, placement by bit counts below.  No atomic decides a place.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"

namespace {
constexpr int BLOCK = 256, TILE = 64, W = NM_STAT_WORDS, PADW = W + 1;
constexpr int VPT = TILE * W / 2 / BLOCK;          // 16-byte pieces of a run per thread
constexpr int G = 4;                               // runs (draws) staged at a time by the chain kernel
constexpr int CC = NM_DIAG_CHAIN_COUNTS, CV = NM_DIAG_CHAIN_VALUES, BINS = NM_DIAG_DEPTH_BINS;
constexpr uint32_t EV_PER_THREAD = 4, EV_BLOCK = BLOCK * EV_PER_THREAD;          // masks per thread / per block of the event kernels
constexpr uint64_t NAN_BITS = 0x7ff8000000000000ull, UNWRITTEN = ~0ull;
static_assert(sizeof(nm_draw_stats) == 8 * W && W % 2 == 0 && TILE * W / 2 == VPT * BLOCK, "a run is whole 16-byte pieces, VPT per thread");
static_assert(G * TILE * PADW * 8 + BINS * TILE * 4 + 64 <= 65536, "the chain kernel's LDS");
enum : int { W_DEPTH = 2, W_MAXDEPTH = 3, W_DIVERGING = 4, W_TUNING = 5, W_NSTEPS = 6, W_STEP = 9, W_ACCEPT = 11, W_LOGP = 14, W_ENERGY = 15, W_STATUS = 19 };
static_assert(offsetof(nm_draw_stats, depth) == 8 * W_DEPTH && offsetof(nm_draw_stats, maxdepth_reached) == 8 * W_MAXDEPTH &&
              offsetof(nm_draw_stats, diverging) == 8 * W_DIVERGING && offsetof(nm_draw_stats, tuning) == 8 * W_TUNING &&
              offsetof(nm_draw_stats, n_steps) == 8 * W_NSTEPS && offsetof(nm_draw_stats, step_size) == 8 * W_STEP &&
              offsetof(nm_draw_stats, mean_tree_accept) == 8 * W_ACCEPT && offsetof(nm_draw_stats, logp) == 8 * W_LOGP &&
              offsetof(nm_draw_stats, energy) == 8 * W_ENERGY && offsetof(nm_draw_stats, chain_status) == 8 * W_STATUS, "word indices");
// which words are doubles, which int64_t (the rest: uint64_t) — the header lists them
constexpr uint32_t DOUBLE_WORDS = (0x3ffu << 9) | (3u << 22), SIGNED_WORDS = (1u << 7) | (1u << 8) | (1u << 20);
static_assert(offsetof(nm_draw_stats, divergence_energy_error) == 8 * 18 && offsetof(nm_draw_stats, energy_change) == 8 * 22 &&
              offsetof(nm_draw_stats, index_in_trajectory) == 8 * 7 && offsetof(nm_draw_stats, transformation_update_id) == 8 * 20, "word kinds");

__device__ inline double dbl(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ inline uint64_t bits(double x) { return (uint64_t)__double_as_longlong(x); }
__device__ inline uint64_t canon(double x) { return x != x ? NAN_BITS : bits(x); }

// the first n_words (even) words at src -> registers: piece v of the run is words 2v, 2v + 1, thread t holds pieces t, t + BLOCK, ...
template <bool WIDE>
__device__ inline void run_load(const uint64_t* src, uint32_t n_words, ulonglong2 (&r)[VPT]) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const uint32_t w = 2u * (threadIdx.x + (uint32_t)k * BLOCK);
        r[k] = make_ulonglong2(0ull, 0ull);
        if (w < n_words) {
            if constexpr (WIDE) {
                r[k] = *reinterpret_cast<const ulonglong2*>(src + w);
            } else {
                r[k].x = src[w];
                r[k].y = src[w + 1];
            }
        }
    }
}

// registers -> the padded LDS image: record i at i * PADW (W is even: a piece never straddles two records)
__device__ inline void run_store(uint64_t* lds, const ulonglong2 (&r)[VPT]) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const uint32_t w = 2u * (threadIdx.x + (uint32_t)k * BLOCK), rec = w / W, f = w - rec * W;
        lds[rec * PADW + f] = r[k].x;
        lds[rec * PADW + f + 1] = r[k].y;
    }
}

struct ColArgs {
    const uint64_t* stats;
    uint64_t* out;
    uint64_t n_rows, n_tiles;
    uint32_t n_fields;
    uint8_t field[W];
};

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void stats_columns_kernel(ColArgs A) {
    __shared__ uint64_t tile[TILE * PADW];
    __shared__ uint32_t fld[W];
    if (threadIdx.x < W) fld[threadIdx.x] = threadIdx.x < A.n_fields ? A.field[threadIdx.x] : 0u;
    const uint32_t nf = A.n_fields;
    for (uint64_t ti = blockIdx.x; ti < A.n_tiles; ti += gridDim.x) {
        const uint64_t row0 = ti * TILE;
        const uint32_t rows = (uint32_t)(A.n_rows - row0 < TILE ? A.n_rows - row0 : TILE);
        ulonglong2 r[VPT];
        run_load<WIDE>(A.stats + row0 * W, rows * W, r);
        __syncthreads();                                   // (the previous run has been read)
        run_store(tile, r);
        __syncthreads();
        uint64_t* const o = A.out + row0 * nf;
        for (uint32_t i = threadIdx.x; i < rows * nf; i += BLOCK) {          // neighbouring threads write neighbouring words
            const uint32_t rec = i / nf, f = fld[i - rec * nf];
            const uint64_t b = tile[rec * PADW + f];
            uint64_t v;
            if (tile[rec * PADW + W_STATUS] == UNWRITTEN) v = NAN_BITS;
            else if ((DOUBLE_WORDS >> f) & 1u) v = b;
            else if ((SIGNED_WORDS >> f) & 1u) v = bits((double)(int64_t)b);
            else v = bits((double)b);
            o[i] = v;
        }
    }
}

struct DiagArgs {
    const uint64_t* stats;
    uint64_t N, C, n_groups;
    uint32_t phase;
    double threshold;
    uint64_t* chain_counts;                  // [C][CC]       the caller's, or scratch
    uint64_t* chain_values;                  // [C][CV]       (bits)
    unsigned long long* pooled_counts;       // [8], zeroed
    unsigned long long* hist;                // [BINS], zeroed
    double* energy;                          // [N][C] scratch: row k holds the k-th selected energy of every chain
    uint64_t* masks;                         // [N][n_groups] or null
};

// The walk over the draws of a block's 64 chains, G runs at a time: the G runs land in LDS, the loads of the next G go out, and wavefront 0
// — a lane is a chain — takes the staged draws in order: per_draw(t, g, the lane's record in LDS).
template <bool WIDE, class F>
__device__ __forceinline__ void walk_draws(const DiagArgs& A, uint64_t (&tiles)[G][TILE * PADW], uint64_t c0, uint32_t chains, F&& per_draw) {
    const uint64_t N = A.N, C = A.C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ulonglong2 r[G][VPT];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if ((uint64_t)g < N) run_load<WIDE>(A.stats + ((uint64_t)g * C + c0) * W, chains * W, r[g]);
    }
    for (uint64_t t0 = 0; t0 < N; t0 += G) {
        __syncthreads();                                   // (the previous draws have been read)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t0 + g < N) run_store(tiles[g], r[g]);
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g) {                      // in flight while wavefront 0 adds up
            if (t0 + G + g < N) run_load<WIDE>(A.stats + ((t0 + G + g) * C + c0) * W, chains * W, r[g]);
        }
        for (int g = 0; wave == 0 && g < G; ++g) {
            if (t0 + g >= N) break;                        // (the same for the whole wavefront)
            per_draw(t0 + g, tiles[g] + lane * PADW);
        }
    }
}

// grid = n_groups: block g owns chains [64 g, 64 g + 64)
template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void diag_chain_kernel(DiagArgs A) {
    __shared__ uint64_t tiles[G][TILE * PADW];
    __shared__ uint32_t hist[BINS][TILE];                  // a column per lane: plain increments, no conflicts
    __shared__ unsigned long long pc[NM_DIAG_POOLED_COUNTS];
    const uint64_t N = A.N, C = A.C, grp = blockIdx.x, c0 = grp * TILE;
    const uint32_t chains = (uint32_t)(C - c0 < TILE ? C - c0 : TILE);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool mine = wave == 0 && (uint32_t)lane < chains;
    const uint64_t c = c0 + (uint64_t)lane;
    for (int i = threadIdx.x; i < BINS * TILE; i += BLOCK) (&hist[0][0])[i] = 0u;
    if (threadIdx.x < NM_DIAG_POOLED_COUNTS) pc[threadIdx.x] = 0ull;
    const uint64_t final_status = mine ? A.stats[((N - 1) * C + c) * W + W_STATUS] : UNWRITTEN;
    const bool healthy = mine && final_status == NM_CHAIN_OK;

    uint64_t k = 0, n_div = 0, n_md = 0, leap = 0, maxd = 0, last_step = NAN_BITS;
    double s_acc = 0.0, s_e = 0.0, s_lp = 0.0, s_d = 0.0, e_prev = 0.0;
    auto selected = [&](const uint64_t* rec) {
        const bool tuning = rec[W_TUNING] != 0;
        return mine && rec[W_STATUS] != UNWRITTEN && (A.phase == NM_DIAG_ALL || (A.phase == NM_DIAG_TUNING) == tuning);
    };

    walk_draws<WIDE>(A, tiles, c0, chains, [&](uint64_t t, const uint64_t* rec) {
        const bool sel = selected(rec);
        const bool div = sel && rec[W_DIVERGING] != 0;
        if (A.masks) {
            const uint64_t m = __ballot(div);
            if (lane == 0) A.masks[t * A.n_groups + grp] = m;
        }
        if (sel) {
            const double e = dbl(rec[W_ENERGY]);
            if (k > 0) {
                const double d = __dsub_rn(e, e_prev);
                s_d = __dadd_rn(s_d, __dmul_rn(d, d));
            }
            e_prev = e;
            s_e = __dadd_rn(s_e, e);
            s_acc = __dadd_rn(s_acc, dbl(rec[W_ACCEPT]));
            s_lp = __dadd_rn(s_lp, dbl(rec[W_LOGP]));
            last_step = rec[W_STEP];
#ifndef NM_DIAG_REREAD_ENERGY
            A.energy[k * C + c] = e;                       // (k <= t < N)
#endif
            ++k;
            n_div += div ? 1 : 0;
            n_md += rec[W_MAXDEPTH] != 0 ? 1 : 0;
            leap += rec[W_NSTEPS];
            const uint64_t depth = rec[W_DEPTH];
            maxd = depth > maxd ? depth : maxd;
            if (healthy) hist[depth < BINS - 1 ? depth : BINS - 1][lane] += 1u;
        }
    });
    const double kd = (double)k;
    const double m = __ddiv_rn(s_e, kd);
    double s_v = 0.0;
#ifdef NM_DIAG_REREAD_ENERGY
    // the measurement variant of DESIGN §31 (tools/build_variant.py): no energy scratch, the records are walked a second time
    walk_draws<WIDE>(A, tiles, c0, chains, [&](uint64_t, const uint64_t* rec) {
        if (selected(rec)) {
            const double d = __dsub_rn(dbl(rec[W_ENERGY]), m);
            s_v = __dadd_rn(s_v, __dmul_rn(d, d));
        }
    });
#else
    if (mine) {
        for (uint64_t j0 = 0; j0 < k; j0 += 8) {           // this lane's own stores, read back; eight loads go out together
            double e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = A.energy[(j0 + j < k ? j0 + j : k - 1) * C + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j0 + j < k) {
                    const double d = __dsub_rn(e[j], m);
                    s_v = __dadd_rn(s_v, __dmul_rn(d, d));
                }
            }
        }
    }
#endif
    if (mine) {
        const double v = __ddiv_rn(s_v, kd);
        const double bfmi = __ddiv_rn(__ddiv_rn(s_d, (double)(k - 1)), v);
        uint64_t* const cc = A.chain_counts + c * CC;
        cc[NM_DIAG_C_ROWS] = k; cc[NM_DIAG_C_DIVERGING] = n_div; cc[NM_DIAG_C_MAXDEPTH] = n_md; cc[NM_DIAG_C_LEAPFROGS] = leap;
        cc[NM_DIAG_C_MAX_DEPTH] = maxd; cc[NM_DIAG_C_FINAL_STATUS] = final_status;
        uint64_t* const cv = A.chain_values + c * CV;
        cv[NM_DIAG_V_MEAN_ACCEPT] = canon(__ddiv_rn(s_acc, kd)); cv[NM_DIAG_V_ENERGY_MEAN] = canon(m); cv[NM_DIAG_V_ENERGY_VAR] = canon(v);
        cv[NM_DIAG_V_BFMI] = canon(bfmi); cv[NM_DIAG_V_MEAN_LOGP] = canon(__ddiv_rn(s_lp, kd)); cv[NM_DIAG_V_LAST_STEP_SIZE] = canon(dbl(last_step));
        if (healthy) {                                     // integer sums: order-free
            atomicAdd(&pc[NM_DIAG_P_HEALTHY], 1ull);
            atomicAdd(&pc[NM_DIAG_P_ROWS], (unsigned long long)k);
            atomicAdd(&pc[NM_DIAG_P_DIVERGING], (unsigned long long)n_div);
            atomicAdd(&pc[NM_DIAG_P_MAXDEPTH], (unsigned long long)n_md);
            atomicAdd(&pc[NM_DIAG_P_LEAPFROGS], (unsigned long long)leap);
            if (n_div) atomicAdd(&pc[NM_DIAG_P_CHAINS_DIVERGING], 1ull);
            if (bfmi < A.threshold) atomicAdd(&pc[NM_DIAG_P_CHAINS_LOW_BFMI], 1ull);
            if (bfmi != bfmi) atomicAdd(&pc[NM_DIAG_P_CHAINS_NAN_BFMI], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < NM_DIAG_POOLED_COUNTS && pc[threadIdx.x]) atomicAdd(&A.pooled_counts[threadIdx.x], pc[threadIdx.x]);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + BINS) {
        const int b = threadIdx.x - 64;
        unsigned long long n = 0;
        for (int l = 0; l < TILE; ++l) n += hist[b][l];
        if (n) atomicAdd(&A.hist[b], n);
    }
}

// thread = chunk of NM_SUMMARY_CHUNK_CHAINS consecutive chains: part[0][chunk], part[1][chunk] the serial sums of MEAN_ACCEPT and
// LAST_STEP_SIZE over its healthy chains, part[2][chunk] the smallest BFMI among them
__global__ __launch_bounds__(BLOCK) void diag_pool_chunks_kernel(const uint64_t* cc, const uint64_t* cv, uint64_t C, uint64_t n_chunks, double* part) {
    const uint64_t chunk = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (chunk >= n_chunks) return;
    const uint64_t first = chunk * NM_SUMMARY_CHUNK_CHAINS, last = first + NM_SUMMARY_CHUNK_CHAINS < C ? first + NM_SUMMARY_CHUNK_CHAINS : C;
    double a = 0.0, s = 0.0, mn = dbl(0x7ff0000000000000ull);
    for (uint64_t c = first; c < last; ++c) {
        if (cc[c * CC + NM_DIAG_C_FINAL_STATUS] != NM_CHAIN_OK) continue;
        a = __dadd_rn(a, dbl(cv[c * CV + NM_DIAG_V_MEAN_ACCEPT]));
        s = __dadd_rn(s, dbl(cv[c * CV + NM_DIAG_V_LAST_STEP_SIZE]));
        const double b = dbl(cv[c * CV + NM_DIAG_V_BFMI]);
        if (b < mn) mn = b;
    }
    part[chunk] = a;
    part[n_chunks + chunk] = s;
    part[2 * n_chunks + chunk] = mn;
}

// one block; thread q < 3 walks the partials of quantity q in chunk order
__global__ __launch_bounds__(64) void diag_pool_finish_kernel(const double* part, uint64_t n_chunks, const unsigned long long* pooled_counts, uint64_t* pooled_values) {
    const int q = threadIdx.x;
    if (q >= NM_DIAG_POOLED_VALUES) return;
    const double* const p = part + (uint64_t)q * n_chunks;
    if (q == NM_DIAG_PV_MIN_BFMI) {
        double mn = dbl(0x7ff0000000000000ull);
        for (uint64_t i = 0; i < n_chunks; ++i) mn = p[i] < mn ? p[i] : mn;
        pooled_values[q] = bits(mn);
    } else {
        double s = 0.0;
        for (uint64_t i = 0; i < n_chunks; ++i) s = __dadd_rn(s, p[i]);
        pooled_values[q] = canon(__ddiv_rn(s, (double)pooled_counts[NM_DIAG_P_HEALTHY]));
    }
}

// ---- the events: masks[M] in (t, group) order; block b owns masks [EV_BLOCK b, EV_BLOCK (b + 1)), a thread EV_PER_THREAD consecutive ones
__device__ inline uint32_t ev_thread_count(const uint64_t* masks, uint64_t M, uint64_t first, uint64_t (&m)[EV_PER_THREAD]) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < EV_PER_THREAD; ++j) {
        m[j] = first + j < M ? masks[first + j] : 0ull;
        n += (uint32_t)__popcll(m[j]);
    }
    return n;
}

__global__ __launch_bounds__(BLOCK) void diag_event_count_kernel(const uint64_t* masks, uint64_t M, uint64_t* block_sum) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    uint64_t m[EV_PER_THREAD];
    const uint32_t n = ev_thread_count(masks, M, (uint64_t)blockIdx.x * EV_BLOCK + (uint64_t)threadIdx.x * EV_PER_THREAD, m);
    if (n) atomicAdd(&total, n);                           // (a count, not a place)
    __syncthreads();
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one block: block_sum becomes its exclusive scan, *n_events the total.  Thread i owns a contiguous piece of the array.
__global__ __launch_bounds__(BLOCK) void diag_event_scan_kernel(uint64_t* block_sum, uint64_t n_blocks, uint64_t* n_events) {
    __shared__ uint64_t piece[BLOCK];
    const uint64_t per = (n_blocks + BLOCK - 1) / BLOCK, first = (uint64_t)threadIdx.x * per;
    const uint64_t last = first + per < n_blocks ? first + per : n_blocks;
    uint64_t s = 0;
    for (uint64_t i = first; i < last; ++i) s += block_sum[i];
    piece[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < BLOCK; ++i) {
            const uint64_t v = piece[i];
            piece[i] = run;
            run += v;
        }
        if (n_events) *n_events = run;
    }
    __syncthreads();
    uint64_t run = piece[threadIdx.x];
    for (uint64_t i = first; i < last; ++i) {
        const uint64_t v = block_sum[i];
        block_sum[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(BLOCK) void diag_event_place_kernel(const uint64_t* masks, uint64_t M, uint64_t n_groups, const uint64_t* block_off,
                                                                 uint64_t* events, uint64_t max_events) {
    __shared__ uint32_t scan[2][BLOCK];
    const int t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * EV_BLOCK + (uint64_t)t * EV_PER_THREAD;
    uint64_t m[EV_PER_THREAD];
    const uint32_t n = ev_thread_count(masks, M, first, m);
    int cur = 0;
    scan[0][t] = n;
    __syncthreads();
    for (int off = 1; off < BLOCK; off <<= 1) {
        const uint32_t v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0u);
        scan[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    uint64_t at = block_off[blockIdx.x] + (uint64_t)(scan[cur][t] - n);          // the events before this thread's first
#pragma unroll
    for (uint32_t j = 0; j < EV_PER_THREAD; ++j) {
        uint64_t mm = m[j];
        if (!mm) continue;
        const uint64_t draw = (first + j) / n_groups, grp = (first + j) - draw * n_groups;
        while (mm) {
            const int b = __ffsll((unsigned long long)mm) - 1;
            mm &= mm - 1;
            if (at < max_events) {                         // nothing is written beyond the capacity
                events[2 * at] = draw;
                events[2 * at + 1] = grp * TILE + (uint64_t)b;
            }
            ++at;
        }
    }
}

thread_local std::string g_derr;
nm_status dfail(const char* call, nm_status st, const std::string& msg) { g_derr = std::string(call) + ": " + msg; return st; }
}  // namespace

extern "C" const char* nm_diag_last_error(void) { return g_derr.c_str(); }

extern "C" nm_status nm_stats_columns(uint64_t n_rows, uint64_t n_fields, const uint64_t* h_fields, const nm_draw_stats* d_stats,
                                      double* d_out, void* stream) {
    const char* const me = "nm_stats_columns";
    // ---- everything that can be refused is refused before the first device call
    if (!h_fields || !d_stats || !d_out) return dfail(me, NM_ERR_INVALID_ARG, "null fields, stats or out");
    if (n_rows == 0) return dfail(me, NM_ERR_INVALID_ARG, "n_rows must be positive");
    if (n_fields == 0 || n_fields > W) return dfail(me, NM_ERR_INVALID_ARG, "n_fields must be 1 .. NM_STAT_WORDS");
    ColArgs A;
    for (uint64_t i = 0; i < W; ++i) A.field[i] = 0;
    for (uint64_t i = 0; i < n_fields; ++i) {
        if (h_fields[i] >= W) return dfail(me, NM_ERR_INVALID_ARG, "field index out of range (0 .. NM_STAT_WORDS - 1)");
        A.field[i] = (uint8_t)h_fields[i];
    }
    {
        typedef unsigned __int128 u128;
        const u128 in0 = (u128)reinterpret_cast<uintptr_t>(d_stats), in1 = in0 + (u128)n_rows * sizeof(nm_draw_stats);
        const u128 o0 = (u128)reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (u128)n_rows * n_fields * 8;
        if (o0 < in1 && in0 < o1) return dfail(me, NM_ERR_INVALID_ARG, "d_out overlaps d_stats");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return dfail(me, NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    A.stats = reinterpret_cast<const uint64_t*>(d_stats);
    A.out = reinterpret_cast<uint64_t*>(d_out);
    A.n_rows = n_rows;
    A.n_tiles = (n_rows + TILE - 1) / TILE;
    A.n_fields = (uint32_t)n_fields;
    const unsigned blocks = (unsigned)(A.n_tiles < 16384 ? A.n_tiles : 16384);
    if ((reinterpret_cast<uintptr_t>(d_stats) & 15) == 0) hipLaunchKernelGGL(stats_columns_kernel<true>, dim3(blocks), dim3(BLOCK), 0, s, A);
    else hipLaunchKernelGGL(stats_columns_kernel<false>, dim3(blocks), dim3(BLOCK), 0, s, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dfail(me, NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}

extern "C" nm_status nm_diagnose_stats(const nm_diag_spec* spec, const nm_draw_stats* d_stats, const nm_diag_outputs* out, void* stream) {
    const char* const me = "nm_diagnose_stats";
    // ---- everything that can be refused is refused before the first device call
    if (!spec || !d_stats || !out) return dfail(me, NM_ERR_INVALID_ARG, "null spec, stats or outputs");
    if (!out->d_chain_counts && !out->d_chain_values && !out->d_pooled_counts && !out->d_pooled_values && !out->d_depth_hist && !out->d_events &&
        !out->d_n_events)
        return dfail(me, NM_ERR_INVALID_ARG, "every output is null");
    const uint64_t N = spec->n_draws, C = spec->n_chains;
    if (N == 0 || C == 0) return dfail(me, NM_ERR_INVALID_ARG, "n_draws and n_chains must be positive");
    if (spec->phase > NM_DIAG_TUNING) return dfail(me, NM_ERR_INVALID_ARG, "unknown phase");
    if (spec->max_events > 0 && !out->d_events) return dfail(me, NM_ERR_INVALID_ARG, "max_events > 0 needs d_events");
    if (spec->bfmi_threshold != spec->bfmi_threshold) return dfail(me, NM_ERR_INVALID_ARG, "bfmi_threshold is NaN");
    if (N > 0xffffffffull / C) return dfail(me, NM_ERR_INVALID_ARG, "more than 2^32 - 1 records");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return dfail(me, NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n_groups = (C + TILE - 1) / TILE, n_chunks = (C + NM_SUMMARY_CHUNK_CHAINS - 1) / NM_SUMMARY_CHUNK_CHAINS;
    const bool events = out->d_n_events || (out->d_events && spec->max_events > 0);
    const uint64_t M = N * n_groups, ev_blocks = (M + EV_BLOCK - 1) / EV_BLOCK;
    // scratch, in 8-byte words: energies [N][C]; zeroed words (pooled counts, histogram); chain counts / values where the caller gives none;
    // chunk partials [3][n_chunks]; pooled values where the caller gives none; masks [M] and block sums
    const uint64_t words = N * C + NM_DIAG_POOLED_COUNTS + BINS + (out->d_chain_counts ? 0 : C * CC) + (out->d_chain_values ? 0 : C * CV) + 3 * n_chunks +
                           (events ? M + ev_blocks : 0);
    uint64_t* scratch = nullptr;
    hipError_t e = hipMallocAsync((void**)&scratch, words * 8, s);
    if (e != hipSuccess) return dfail(me, NM_ERR_HIP, hipGetErrorString(e));
    uint64_t* p = scratch;
    DiagArgs A;
    A.energy = reinterpret_cast<double*>(p); p += N * C;
    uint64_t* const zeroed = p; p += NM_DIAG_POOLED_COUNTS + BINS;
    A.pooled_counts = out->d_pooled_counts ? static_cast<unsigned long long*>(out->d_pooled_counts) : reinterpret_cast<unsigned long long*>(zeroed);
    A.hist = out->d_depth_hist ? static_cast<unsigned long long*>(out->d_depth_hist) : reinterpret_cast<unsigned long long*>(zeroed + NM_DIAG_POOLED_COUNTS);
    if (out->d_chain_counts) A.chain_counts = static_cast<uint64_t*>(out->d_chain_counts); else { A.chain_counts = p; p += C * CC; }
    if (out->d_chain_values) A.chain_values = reinterpret_cast<uint64_t*>(out->d_chain_values); else { A.chain_values = p; p += C * CV; }
    double* const part = reinterpret_cast<double*>(p); p += 3 * n_chunks;
    A.masks = events ? p : nullptr;
    uint64_t* const block_sum = events ? p + M : nullptr;
    A.stats = reinterpret_cast<const uint64_t*>(d_stats);
    A.N = N; A.C = C; A.n_groups = n_groups; A.phase = (uint32_t)spec->phase; A.threshold = spec->bfmi_threshold;

    e = hipMemsetAsync(zeroed, 0, (NM_DIAG_POOLED_COUNTS + BINS) * 8, s);
    if (e == hipSuccess && out->d_pooled_counts) e = hipMemsetAsync(out->d_pooled_counts, 0, NM_DIAG_POOLED_COUNTS * 8, s);
    if (e == hipSuccess && out->d_depth_hist) e = hipMemsetAsync(out->d_depth_hist, 0, BINS * 8, s);
    if (e == hipSuccess) {
        if ((reinterpret_cast<uintptr_t>(d_stats) & 15) == 0) hipLaunchKernelGGL(diag_chain_kernel<true>, dim3((unsigned)n_groups), dim3(BLOCK), 0, s, A);
        else hipLaunchKernelGGL(diag_chain_kernel<false>, dim3((unsigned)n_groups), dim3(BLOCK), 0, s, A);
        if (out->d_pooled_values) {
            hipLaunchKernelGGL(diag_pool_chunks_kernel, dim3((unsigned)((n_chunks + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                               (const uint64_t*)A.chain_counts, (const uint64_t*)A.chain_values, C, n_chunks, part);
            hipLaunchKernelGGL(diag_pool_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)part, n_chunks,
                               (const unsigned long long*)A.pooled_counts, reinterpret_cast<uint64_t*>(out->d_pooled_values));
        }
        if (events) {
            hipLaunchKernelGGL(diag_event_count_kernel, dim3((unsigned)ev_blocks), dim3(BLOCK), 0, s, (const uint64_t*)A.masks, M, block_sum);
            hipLaunchKernelGGL(diag_event_scan_kernel, dim3(1), dim3(BLOCK), 0, s, block_sum, ev_blocks, static_cast<uint64_t*>(out->d_n_events));
            if (out->d_events && spec->max_events > 0)
                hipLaunchKernelGGL(diag_event_place_kernel, dim3((unsigned)ev_blocks), dim3(BLOCK), 0, s, (const uint64_t*)A.masks, M, n_groups,
                                   (const uint64_t*)block_sum, static_cast<uint64_t*>(out->d_events), spec->max_events);
        }
        e = hipGetLastError();
    }
    (void)hipFreeAsync(scratch, s);
    if (e != hipSuccess) return dfail(me, NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}
