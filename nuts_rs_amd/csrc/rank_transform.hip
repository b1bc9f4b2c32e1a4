// rank_transform.hip — rank transforms of a recorded trace on the device (nm_transform_draws, include/nuts_amd.h): per element the normal
// scores of the pooled ranks (plain or folded about a centre) or an indicator, written compact over the selected chains so that
// nm_summarize_draws turns them into rank-normalised R-hat and bulk / tail ESS.  NOT reference behaviour: the definition is this
// repository's, the header states it, tests/rank_ref.py restates it in numpy with the same bits.
//
// A post-pass over buffers the draw calls have written; engine-free, no draw kernel is involved.  The ranks of ALL elements of a column
// need the column sorted: a segmented least-significant-digit radix sort of (key, pool index) pairs, 8 passes of 8 bits, in batches of as
// many columns as the scratch budget holds:
//   gather kernel   reads contiguous runs of `row * dim + col` (16 B per lane where the trace allows it), applies the fold, writes keys
//                   and pool indices column-major into scratch, counts NaNs.
//   count kernel    per pass: a block owns a slab of NM_RANK_SLAB_KEYS consecutive positions of one column, each of its wavefronts a
//                   quarter of it; it writes the slab's digit counts to table[column][digit][slab].
//   scan kernel     per pass: one block per column, an exclusive scan of that table, digit-major and slab-minor.
//   scatter kernel  per pass, STABLE: the block counts its wavefronts' quarters again, which gives per-wavefront digit counters in LDS;
//                   every wavefront then walks its quarter in order, 64 keys at a time: the lanes that share a digit find each other
//                   with one __ballot per digit bit, a lane's place is counter + popcount(peers below it), the lowest lane of a peer
//                   group bumps the counter.  No atomic decides a position.  The places are places INSIDE the slab first (a 16-bit
//                   permutation in LDS); the block then writes place by place, so that a digit's run leaves as whole cache lines.
//   score kernel    position p of the sorted column looks at its neighbours: no equal neighbour, a = p and b = p + 1; else the tie run's
//                   ends by binary search (only ties pay); rank2 = a + b + 1, the score, scattered to the element's place.
//   indicator kernel (kind 2) elementwise, no sort.
// Every number that decides anything is an integer count: the bits do not depend on the grid, the batching or arrival order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"
#include "rank_score.hpp"

namespace {
constexpr int BLOCK = 256, WAVES = BLOCK / 64, DIGITS = 256, PASSES = 8;
constexpr uint32_t SLAB = NM_RANK_SLAB_KEYS, SUB = SLAB / WAVES;          // a wavefront's quarter of a slab
static_assert(SUB % 512 == 0 && SLAB <= 16384, "a wavefront walks whole rounds of 64 keys, eight rounds of loads at a time");
constexpr int TILE_COLS = 16;          // the gather's column tile: 128 B runs read, 32 rows side by side
constexpr int GROWS = 4;               // rounds of rows per gather block
constexpr uint64_t MAX_BATCH_COLS = 32768;          // (the column is a grid's y)
constexpr uint64_t NAN_BITS = 0x7ff8000000000000ull, ABS_MASK = 0x7fffffffffffffffull, INF_BITS = 0x7ff0000000000000ull;

__device__ inline uint64_t key_of(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull); }

struct GatherArgs {
    const double* x;                    // [N][C][D]
    const double* param;                // [D], read when fold
    const uint64_t* ids;                // device, [csel] or null
    uint64_t* keys;                     // [ncols][n]
    uint32_t* idx;                      // [ncols][n]
    uint32_t* nan;                      // [D]
    uint64_t dim, chains, csel, n, half, skip, col0, ncols;          // skip: the draw `half` is not in the pool
    int fold, tile_cols, tile_vecs, groups;
};

template <int V>
__global__ __launch_bounds__(BLOCK) void rank_gather_kernel(GatherArgs A) {
    const int t = threadIdx.x, g = t / A.tile_vecs, lv = t - g * A.tile_vecs;
    const uint64_t lc = (uint64_t)blockIdx.y * A.tile_cols + (uint64_t)lv * V;          // column inside the batch
    if (g >= A.groups || lc >= A.ncols) return;
    const uint64_t col = A.col0 + lc;
    double c[V];
#pragma unroll
    for (int j = 0; j < V; ++j) c[j] = (A.fold && lc + j < A.ncols) ? A.param[col + j] : 0.0;
    for (int u = 0; u < GROWS; ++u) {
        const uint64_t p = ((uint64_t)blockIdx.x * GROWS + u) * A.groups + g;          // pool index
        if (p >= A.n) break;
        const uint64_t pr = p / A.csel, cs = p - pr * A.csel;
        const uint64_t draw = pr + ((A.skip && pr >= A.half) ? 1 : 0);
        const uint64_t chain = A.ids ? A.ids[cs] : cs;
        const uint64_t at = (draw * A.chains + chain) * A.dim + col;
        uint64_t b[V];
        if constexpr (V == 2) {          // (dim and col are even: col + 1 is a column of the trace, and the run is 16-byte aligned)
            const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(A.x + at);
            b[0] = q.x; b[1] = q.y;
        } else {
            b[0] = *reinterpret_cast<const uint64_t*>(A.x + at);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (lc + j >= A.ncols) continue;
            uint64_t bits = b[j];
            if (A.fold) bits = (uint64_t)__double_as_longlong(__dsub_rn(__longlong_as_double((long long)bits), c[j])) & ABS_MASK;
            if ((bits & ABS_MASK) > INF_BITS) atomicAdd(&A.nan[col + j], 1u);
            A.keys[(lc + j) * A.n + p] = key_of(bits);
            A.idx[(lc + j) * A.n + p] = (uint32_t)p;
        }
    }
}

// cnt[w][digit] = how many keys of wavefront w's quarter of the slab carry the digit (integer LDS adds: a count, not a position)
// KEEP: the lane also keeps the digits of its keys, four to a word (round `it` in byte it % 4 of dig[it / 4]): the scatter kernel
// walks them again without a second trip to memory
constexpr int ROUNDS = SUB / 64, DIG_WORDS = (ROUNDS + 3) / 4;
template <bool KEEP>
__device__ inline void count_quarters(const uint64_t* keys, uint64_t n, uint64_t slab, int shift, uint32_t* cnt, uint32_t (&dig)[DIG_WORDS]) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int i = t; i < WAVES * DIGITS; i += BLOCK) cnt[i] = 0;
#pragma unroll
    for (int i = 0; i < DIG_WORDS; ++i) dig[i] = 0;
    __syncthreads();
    const uint64_t base = slab * SLAB + (uint64_t)w * SUB + lane;
#pragma unroll
    for (int it0 = 0; it0 < ROUNDS; it0 += 8) {
        uint64_t key[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                              // (read unconditionally: the eight loads go out together)
            const uint64_t pos = base + (uint32_t)(it0 + j) * 64u;
            key[j] = keys[pos < n ? pos : n - 1];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t pos = base + (uint32_t)(it0 + j) * 64u;
            const uint32_t digit = (uint32_t)(key[j] >> shift) & 255u;
            if (pos < n) atomicAdd(&cnt[w * DIGITS + (int)digit], 1u);
            if (KEEP) dig[(it0 + j) / 4] |= digit << (8 * ((it0 + j) % 4));
        }
    }
    __syncthreads();
}

// grid (slabs, columns)
__global__ __launch_bounds__(BLOCK) void rank_count_kernel(const uint64_t* keys, uint32_t* table, uint64_t n, uint64_t slabs, int shift) {
    __shared__ uint32_t cnt[WAVES * DIGITS];
    const uint64_t col = blockIdx.y, slab = blockIdx.x;
    uint32_t dig[DIG_WORDS];
    count_quarters<false>(keys + col * n, n, slab, shift, cnt, dig);
    const int d = threadIdx.x;
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += cnt[w * DIGITS + d];
    table[(col * DIGITS + d) * slabs + slab] = total;
}

// one block per column, thread d = digit d: the table becomes its exclusive scan in (digit, slab) order
__global__ __launch_bounds__(DIGITS) void rank_scan_kernel(uint32_t* table, uint64_t slabs) {
    __shared__ uint32_t scan[2][DIGITS];
    const int d = threadIdx.x;
    uint32_t* const row = table + ((uint64_t)blockIdx.x * DIGITS + d) * slabs;
    uint32_t sum = 0;
#pragma unroll 8
    for (uint64_t s = 0; s < slabs; ++s) sum += row[s];
    int cur = 0;
    scan[0][d] = sum;
    __syncthreads();
    for (int off = 1; off < DIGITS; off <<= 1) {
        const uint32_t v = scan[cur][d] + (d >= off ? scan[cur][d - off] : 0u);
        scan[cur ^ 1][d] = v;
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = scan[cur][d] - sum;
#pragma unroll 8
    for (uint64_t s = 0; s < slabs; ++s) {
        const uint32_t c = row[s];
        row[s] = run;
        run += c;
    }
}

// grid (slabs, columns); the pass is stable: equal digits keep their order.  The block first puts its slab in digit order INSIDE the slab
// (perm: local place -> offset in the slab), then writes it out place by place: neighbouring threads write neighbouring words of a digit's
// run (32 keys on average) instead of 64 keys of a wavefront going to 64 cache lines.
__global__ __launch_bounds__(BLOCK) void rank_scatter_kernel(const uint64_t* kin, const uint32_t* iin, uint64_t* kout, uint32_t* iout,
                                                             const uint32_t* table, uint64_t n, uint64_t slabs, int shift) {
    __shared__ uint32_t cnt[WAVES * DIGITS];
    __shared__ uint32_t scan[2][DIGITS];
    __shared__ uint32_t gbase[DIGITS];          // place in the column = gbase[digit] + place in the slab (modulo 2^32)
    __shared__ uint16_t perm[SLAB];
    const uint64_t col = blockIdx.y, slab = blockIdx.x;
    kin += col * n; iin += col * n; kout += col * n; iout += col * n;
    uint32_t dig[DIG_WORDS];
    count_quarters<true>(kin, n, slab, shift, cnt, dig);
    {
        const int d = threadIdx.x;
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) total += cnt[w * DIGITS + d];
        int cur = 0;
        scan[0][d] = total;
        __syncthreads();
        for (int off = 1; off < DIGITS; off <<= 1) {
            const uint32_t v = scan[cur][d] + (d >= off ? scan[cur][d - off] : 0u);
            scan[cur ^ 1][d] = v;
            cur ^= 1;
            __syncthreads();
        }
        const uint32_t lbase = scan[cur][d] - total;          // the slab's keys of smaller digits
        gbase[d] = table[(col * DIGITS + d) * slabs + slab] - lbase;
        uint32_t run = lbase;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = cnt[w * DIGITS + d];
            cnt[w * DIGITS + d] = run;          // the place in the slab of wavefront w's first key of this digit
            run += c;
        }
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // this wavefront's counters: nobody else touches them from here on.  Lanes hand values to each other through them: relaxed atomic
    // accesses (plain ds_read / ds_write, which a wavefront's LDS pipeline runs in order) between wavefront-scope fences
    uint32_t* const ctr = cnt + w * DIGITS;
    const uint64_t slab0 = slab * SLAB;
    const uint32_t slab_n = (uint32_t)(n - slab0 < SLAB ? n - slab0 : SLAB);
    const uint64_t below_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int it = 0; it < ROUNDS; ++it) {                            // (unrolled: the digits sit in registers)
        const uint32_t src0 = (uint32_t)w * SUB + (uint32_t)it * 64u;          // offset in the slab
        if (src0 >= slab_n) break;                                   // (the same for the whole wavefront)
        const uint32_t src = src0 + lane;
        const bool valid = src < slab_n;
        const uint32_t digit = (dig[it / 4] >> (8 * (it % 4))) & 255u;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t below = (uint32_t)__popcll(peers & below_mask);
        const uint32_t off = valid ? __hip_atomic_load(&ctr[digit], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // every lane has read its counter before a leader rewrites it
        if (valid && below == 0) __hip_atomic_store(&ctr[digit], off + (uint32_t)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t place = off + below;
        if (valid && place < SLAB) perm[place] = (uint16_t)src;      // (place < slab_n whenever the counts are this pass's: a guard)
    }
    __syncthreads();
    for (uint32_t place0 = threadIdx.x; place0 < slab_n; place0 += BLOCK * 4) {
        uint64_t key[4];
        uint32_t id[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                 // (four reads in flight; a place past the slab reads the slab's first pair)
            const uint32_t place = place0 + (uint32_t)j * BLOCK;
            uint32_t src = place < slab_n ? perm[place] : 0u;
            src = src < slab_n ? src : 0u;                            // (always: a guard against a stray read)
            key[j] = kin[slab0 + src];
            id[j] = iin[slab0 + src];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t place = place0 + (uint32_t)j * BLOCK;
            const uint32_t dst = gbase[(uint32_t)(key[j] >> shift) & 255u] + place;
            if (place < slab_n && dst < n) {                          // (dst < n always, with this pass's table: a guard against a stray write)
                kout[dst] = key[j];
                iout[dst] = id[j];
            }
        }
    }
}

struct ScoreArgs {
    const uint64_t* keys;               // [ncols][n], sorted
    const uint32_t* idx;
    const uint32_t* nan;                // [D]
    double* out;                        // [N][csel][D] or null
    uint32_t* rank2;                    // the same shape, or null
    uint64_t* nan_count;                // [D] or null
    uint64_t n, csel, dim, half, skip, col0;
};

// grid (ceil(n / BLOCK), columns)
__global__ __launch_bounds__(BLOCK) void rank_score_kernel(ScoreArgs A) {
    nm::dm_init_lds();                                          // dlog's tables
    const uint64_t lc = blockIdx.y, col = A.col0 + lc, p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, n = A.n;
    const uint32_t n_nan = A.nan[col];
    if (p == 0 && A.nan_count) A.nan_count[col] = n_nan;
    if (p >= n) return;
    const uint64_t* const K = A.keys + lc * n;
    const uint64_t key = K[p];
    uint64_t a = p, b = p + 1;
    if (p > 0 && K[p - 1] == key) {                             // the first position of the tie run
        uint64_t lo = 0, hi = p - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (K[mid] < key) lo = mid + 1; else hi = mid;
        }
        a = lo;
    }
    if (p + 1 < n && K[p + 1] == key) {                         // one past its last position
        uint64_t lo = p + 2, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (K[mid] <= key) lo = mid + 1; else hi = mid;
        }
        b = lo;
    }
    const uint64_t r2 = a + b + 1;
    const uint64_t e = A.idx[lc * n + p];
    if (e >= n) return;                                         // (never: a guard against a stray write)
    const uint64_t pr = e / A.csel, cs = e - pr * A.csel;
    const uint64_t draw = pr + ((A.skip && pr >= A.half) ? 1 : 0);
    const uint64_t o = (draw * A.csel + cs) * A.dim + col;
    if (A.out) A.out[o] = n_nan ? __longlong_as_double((long long)NAN_BITS) : nm::rank_normal_score(n, r2);
    if (A.rank2) A.rank2[o] = n_nan ? 0u : (uint32_t)r2;
}

// the draw that is in no split half: NaN and 0 in every selected chain and column
__global__ __launch_bounds__(BLOCK) void rank_fill_row_kernel(double* out, uint32_t* rank2, uint64_t first, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    if (out) out[first + i] = __longlong_as_double((long long)NAN_BITS);
    if (rank2) rank2[first + i] = 0u;
}

__global__ __launch_bounds__(BLOCK) void rank_indicator_kernel(const double* x, const double* param, const uint64_t* ids, double* out,
                                                               unsigned long long* nan_count, uint64_t total, uint64_t dim, uint64_t chains, uint64_t csel) {
    for (uint64_t o = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; o < total; o += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t rc = o / dim, d = o - rc * dim;
        const uint64_t draw = rc / csel, cs = rc - draw * csel;
        const uint64_t chain = ids ? ids[cs] : cs;
        const double v = x[(draw * chains + chain) * dim + d], c = param[d];
        double r = v <= c ? 1.0 : 0.0;
        if (v != v) {
            r = v;
            if (nan_count) atomicAdd(&nan_count[d], 1ull);          // (an integer count)
        }
        if (c != c) r = c;
        if (r != r) r = __longlong_as_double((long long)NAN_BITS);
        out[o] = r;
    }
}

thread_local std::string g_terr;
nm_status tfail(nm_status st, const std::string& msg) { g_terr = "nm_transform_draws: " + msg; return st; }
}  // namespace

extern "C" const char* nm_transform_last_error(void) { return g_terr.c_str(); }

extern "C" nm_status nm_rank_normal_score(uint64_t n, uint64_t rank2, double* z) {
    if (!z) { g_terr = "nm_rank_normal_score: null z"; return NM_ERR_INVALID_ARG; }
    if (n == 0 || n > 0x7fffffffull || rank2 < 2 || rank2 > 2 * n) { g_terr = "nm_rank_normal_score: n must be 1 .. 2^31 - 1 and rank2 2 .. 2n"; return NM_ERR_INVALID_ARG; }
    *z = nm::rank_normal_score(n, rank2);
    return NM_OK;
}

extern "C" nm_status nm_transform_draws(const nm_transform_spec* spec, const double* d_draws, const double* d_param,
                                        const nm_transform_outputs* out, void* stream) {
    // ---- everything that can be refused is refused before the first device call
    if (!spec || !d_draws || !out) return tfail(NM_ERR_INVALID_ARG, "null spec, draws or outputs");
    if (!out->d_out && !out->d_rank2) return tfail(NM_ERR_INVALID_ARG, "d_out and d_rank2 are both null");
    const uint64_t kind = spec->kind;
    if (kind > NM_TRANSFORM_INDICATOR_LE) return tfail(NM_ERR_INVALID_ARG, "unknown kind");
    if (spec->split > 1) return tfail(NM_ERR_INVALID_ARG, "split must be 0 or 1");
    if (kind != NM_TRANSFORM_RANK_NORMAL && !d_param) return tfail(NM_ERR_INVALID_ARG, "this kind needs d_param");
    if (kind == NM_TRANSFORM_INDICATOR_LE && out->d_rank2) return tfail(NM_ERR_INVALID_ARG, "the indicator has no ranks: d_rank2 must be null");
    const uint64_t N = spec->n_draws, C = spec->n_chains, D = spec->dim;
    if (N == 0 || C == 0 || D == 0) return tfail(NM_ERR_INVALID_ARG, "n_draws, n_chains and dim must be positive");
    uint64_t csel = C;
    const uint64_t* h_ids = static_cast<const uint64_t*>(spec->h_chain_ids);
    if (h_ids) {
        csel = spec->n_chain_ids;
        if (csel == 0) return tfail(NM_ERR_INVALID_ARG, "no chain selected");
        for (uint64_t i = 0; i < csel; ++i) {
            if (h_ids[i] >= C) return tfail(NM_ERR_INVALID_ARG, "chain id out of range");
            if (i && h_ids[i] <= h_ids[i - 1]) return tfail(NM_ERR_INVALID_ARG, "chain ids must be strictly increasing");
        }
    }
    const bool skip = spec->split == 1 && N % 2 == 1;
    const uint64_t pool_rows = skip ? N - 1 : N, half = N / 2;
    if (pool_rows == 0) return tfail(NM_ERR_INVALID_ARG, "the pool is empty (one draw, split)");
    if (pool_rows > 0x7fffffffull / csel) return tfail(NM_ERR_INVALID_ARG, "more than 2^31 - 1 pooled values per element");
    const uint64_t n = pool_rows * csel;
    if (D > 0x7fffffffull) return tfail(NM_ERR_INVALID_ARG, "dim above 2^31 - 1");
    if (out->d_out) {
        typedef unsigned __int128 u128;
        const u128 in0 = (u128)reinterpret_cast<uintptr_t>(d_draws), in1 = in0 + (u128)N * C * D * 8;
        const u128 o0 = (u128)reinterpret_cast<uintptr_t>(out->d_out), o1 = o0 + (u128)N * csel * D * 8;
        if (o0 < in1 && in0 < o1) return tfail(NM_ERR_INVALID_ARG, "d_out overlaps d_draws");
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return tfail(NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n_ids = h_ids ? csel : 0;
    hipError_t e;
    auto upload_ids = [&](uint64_t* d_ids) {
        hipError_t r = hipMemcpyAsync(d_ids, h_ids, n_ids * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);          // the caller's array is free on return
        return r;
    };

    if (kind == NM_TRANSFORM_INDICATOR_LE) {
        uint64_t* d_ids = nullptr;
        if (n_ids) {
            e = hipMallocAsync((void**)&d_ids, n_ids * sizeof(uint64_t), s);
            if (e != hipSuccess) return tfail(NM_ERR_HIP, hipGetErrorString(e));
            e = upload_ids(d_ids);
            if (e != hipSuccess) { (void)hipFreeAsync(d_ids, s); return tfail(NM_ERR_HIP, hipGetErrorString(e)); }
        }
        e = out->d_nan_count ? hipMemsetAsync(out->d_nan_count, 0, D * sizeof(uint64_t), s) : hipSuccess;
        if (e == hipSuccess) {
            const uint64_t total = N * csel * D;
            const uint64_t blocks = std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 16384);
            hipLaunchKernelGGL(rank_indicator_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, d_draws, d_param, d_ids, out->d_out,
                               static_cast<unsigned long long*>(out->d_nan_count), total, D, C, csel);
            e = hipGetLastError();
        }
        if (d_ids) (void)hipFreeAsync(d_ids, s);
        if (e != hipSuccess) return tfail(NM_ERR_HIP, hipGetErrorString(e));
        return NM_OK;
    }

    // ---- the rank kinds: column batches that fit the scratch budget
    const uint64_t slabs = (n + SLAB - 1) / SLAB;
    const uint64_t per_col = 24 * n + (uint64_t)DIGITS * 4 * slabs;
    const uint64_t budget = spec->max_scratch_bytes ? spec->max_scratch_bytes : (1ull << 30);
    const bool wide = D % 2 == 0 && (reinterpret_cast<uintptr_t>(d_draws) & 15) == 0;
    uint64_t cols = std::min<uint64_t>(std::max<uint64_t>(budget / per_col, 1), std::min<uint64_t>(D, MAX_BATCH_COLS));
    if (wide && cols > 1 && cols % 2 == 1) --cols;          // (even batches: every batch of a wide trace starts at an even column)
    // scratch, 8-byte words first: keys A, keys B [cols][n], (ids [csel]); then 4-byte words: idx A, idx B [cols][n], table [cols][256][slabs], nan [D]
    const uint64_t bytes = (2 * cols * n + n_ids) * 8 + (2 * cols * n + cols * DIGITS * slabs + D) * 4;
    char* scratch = nullptr;
    e = hipMallocAsync((void**)&scratch, bytes, s);
    if (e != hipSuccess) return tfail(NM_ERR_HIP, hipGetErrorString(e));
    uint64_t* const keys_a = reinterpret_cast<uint64_t*>(scratch);
    uint64_t* const keys_b = keys_a + cols * n;
    uint64_t* const d_ids = n_ids ? keys_b + cols * n : nullptr;
    uint32_t* const idx_a = reinterpret_cast<uint32_t*>(keys_b + cols * n + n_ids);
    uint32_t* const idx_b = idx_a + cols * n;
    uint32_t* const table = idx_b + cols * n;
    uint32_t* const nan = table + cols * DIGITS * slabs;
    if (n_ids) {
        e = upload_ids(d_ids);
        if (e != hipSuccess) { (void)hipFreeAsync(scratch, s); return tfail(NM_ERR_HIP, hipGetErrorString(e)); }
    }
    e = hipMemsetAsync(nan, 0, D * sizeof(uint32_t), s);
    if (e != hipSuccess) { (void)hipFreeAsync(scratch, s); return tfail(NM_ERR_HIP, hipGetErrorString(e)); }
    double* const d_out = out->d_out;
    uint32_t* const d_rank2 = static_cast<uint32_t*>(out->d_rank2);
    if (skip) {
        const uint64_t count = csel * D;
        hipLaunchKernelGGL(rank_fill_row_kernel, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, d_out, d_rank2, half * count, count);
    }
    for (uint64_t col0 = 0; col0 < D; col0 += cols) {
        const uint64_t nc = std::min(cols, D - col0);
        GatherArgs G;
        G.x = d_draws; G.param = d_param; G.ids = d_ids; G.keys = keys_a; G.idx = idx_a; G.nan = nan;
        G.dim = D; G.chains = C; G.csel = csel; G.n = n; G.half = half; G.skip = skip ? 1 : 0; G.col0 = col0; G.ncols = nc;
        G.fold = kind == NM_TRANSFORM_FOLDED_RANK_NORMAL ? 1 : 0;
        const int V = (wide && col0 % 2 == 0) ? 2 : 1;
        const uint64_t tile_cols = std::min<uint64_t>((nc + V - 1) / V * V, TILE_COLS);
        G.tile_cols = (int)tile_cols;
        G.tile_vecs = (int)(tile_cols / V);
        G.groups = BLOCK / G.tile_vecs;
        const uint64_t rows_per_block = (uint64_t)G.groups * GROWS;
        const dim3 ggrid((unsigned)((n + rows_per_block - 1) / rows_per_block), (unsigned)((nc + tile_cols - 1) / tile_cols));
        if (V == 2) hipLaunchKernelGGL(rank_gather_kernel<2>, ggrid, dim3(BLOCK), 0, s, G);
        else hipLaunchKernelGGL(rank_gather_kernel<1>, ggrid, dim3(BLOCK), 0, s, G);
        const dim3 sgrid((unsigned)slabs, (unsigned)nc);
        for (int pass = 0; pass < PASSES; ++pass) {
            const bool fwd = pass % 2 == 0;
            const uint64_t* kin = fwd ? keys_a : keys_b;
            const uint32_t* iin = fwd ? idx_a : idx_b;
            hipLaunchKernelGGL(rank_count_kernel, sgrid, dim3(BLOCK), 0, s, kin, table, n, slabs, 8 * pass);
            hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)nc), dim3(DIGITS), 0, s, table, slabs);
            hipLaunchKernelGGL(rank_scatter_kernel, sgrid, dim3(BLOCK), 0, s, kin, iin, fwd ? keys_b : keys_a, fwd ? idx_b : idx_a,
                               (const uint32_t*)table, n, slabs, 8 * pass);
        }
        // (an even number of passes: the sorted pairs are back in A)
        ScoreArgs S;
        S.keys = keys_a; S.idx = idx_a; S.nan = nan; S.out = d_out; S.rank2 = d_rank2; S.nan_count = static_cast<uint64_t*>(out->d_nan_count);
        S.n = n; S.csel = csel; S.dim = D; S.half = half; S.skip = skip ? 1 : 0; S.col0 = col0;
        hipLaunchKernelGGL(rank_score_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK), (unsigned)nc), dim3(BLOCK), 0, s, S);
    }
    e = hipGetLastError();
    (void)hipFreeAsync(scratch, s);
    if (e != hipSuccess) return tfail(NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}
