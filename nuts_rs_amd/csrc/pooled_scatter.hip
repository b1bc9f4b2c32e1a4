// pooled_scatter.hip — nm_pooled_scatter (include/nuts_amd.h): the centred scatter matrix S = sum (x - c)(x - c)' of a window
// of recorded rows on the f64 matrix cores.  NOT reference behaviour: it is the device half of the pooled LOW-RANK adaptation
// (nuts_rs_amd/pooled.py; the reference's estimate, src/transform/adapt/low_rank.rs:73-262, needs of a window only its count, means and
// the scatter matrices of draws and gradients), and the covariance of a trace.  The definition is the header's; tests/scatter_ref.py
// restates it with the same bits.
//
// Engine-free, a post-pass like nm_pooled_partials.
//   scatter kernel  grid (upper-triangle macro tiles, slabs), 4 wavefronts.  A block owns the 64 x 64 outputs (i0 .., j0 ..), j0 >= i0, of
//                   ONE slab of rows and streams the slab through LDS in panels of 32 rows: columns i0 .. i0 + 63 and j0 .. j0 + 63 of the
//                   rows, centred on the way in (one rounded subtraction), +0.0 where the row is left out, beyond the slab's end or the
//                   column beyond dim — fma(+0, +0, acc) leaves acc as it is, so padding moves no bit.  Both MFMA operands are the SAME
//                   access: lane l reads Y[k0 + (l >> 4)][col0 + (l & 15)] — A is Y', B is Y, no transpose is staged — and a diagonal
//                   macro tile keeps one panel for both.  Wavefront w owns the 16-row stripe w of the tile: four independent 16 x 16
//                   accumulators, interleaved, each an fma chain over the slab's rows in row order (v_mfma_f64_16x16x4_f64 is that chain
//                   over k ascending).  The next panel's rows are in flight (registers) while the current one is multiplied.
//   merge kernel    adds the slab partials in slab order from +0.0, writes S[i][j] and its mirror, and the count.
// One accumulator per output and slab, k-steps in row order, slabs cut by n_rows alone: the same rows give the same bits whatever the grid.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"
#include "pooled_rows.hpp"

namespace {
using nm::pooled::row_ok;
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int TILE = 64;             // outputs of a macro tile per side
constexpr int KP = 32;               // rows of a panel
constexpr int LDW = 80;              // doubles per panel row in LDS: 64 + 16, so that the four rows of an operand read (lanes l >> 4) fall on different banks
constexpr int THREADS = 256;

struct ScatterArgs {
    const double* x;                 // [n_rows][dim]
    const double* c;                 // [dim]
    const nm_draw_stats* st;         // [n_rows] or null
    double* partial;                 // [n_slabs][n_upper][64][64]
    double* slab_count;              // [n_slabs]: kept rows per slab (written when st is given)
    uint64_t n_rows, dim, slab_rows;
    unsigned tiles, n_upper;         // T = ceil(dim / 64); T (T + 1) / 2
};

// upper-triangle tile number -> (ti, tj), row by row
__device__ inline void tile_of(unsigned u, unsigned T, unsigned& ti, unsigned& tj) {
    ti = 0;
    while (u >= T - ti) { u -= T - ti; ++ti; }
    tj = ti + u;
}

// a thread's share of a panel: rows rr + 8 u, u = 0 .. 3, columns col, col + 1 (raw values; nothing is read where the select below takes +0.0)
template <bool V2>
__device__ inline void fetch(const double* x, uint64_t dim, uint64_t row0, unsigned keep, uint64_t col, int rr, double (&raw)[8]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double* p = x + (row0 + (uint64_t)(rr + 8 * u)) * dim + col;
        double a = 0.0, b = 0.0;
        if ((keep >> u) & 1u) {
            if constexpr (V2) {
                if (col < dim) { const double2 q = *reinterpret_cast<const double2*>(p); a = q.x; b = q.y; }       // (dim is even: col + 1 < dim)
            } else {
                if (col < dim) a = p[0];
                if (col + 1 < dim) b = p[1];
            }
        }
        raw[2 * u] = a; raw[2 * u + 1] = b;
    }
}
// centred on the way into LDS; +0.0 for a row that is left out or beyond the slab, and for a column beyond dim
__device__ inline void stage(double* panel, unsigned keep, bool ok0, bool ok1, double c0, double c1, int rr, int cp, const double (&raw)[8]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool k = (keep >> u) & 1u;
        const double y0 = raw[2 * u] - c0, y1 = raw[2 * u + 1] - c1;
        *reinterpret_cast<double2*>(panel + (rr + 8 * u) * LDW + 2 * cp) = make_double2(k && ok0 ? y0 : 0.0, k && ok1 ? y1 : 0.0);
    }
}

// One panel on the matrix cores: NA independent 16 x 16 accumulators of a wavefront's stripe, interleaved; rows 4 ks .. 4 ks + 3 of the panel
// per instruction, k ascending inside it.
template <int NA>
__device__ inline void mma_panel(const double* ai, const double* bj, v4d (&acc)[4]) {
#pragma unroll
    for (int ks = 0; ks < KP / 4; ++ks) {
        const double a = ai[4 * ks * LDW];
        double b[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) b[q] = bj[4 * ks * LDW + 16 * q];
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc[q], 0, 0, 0);
    }
}

template <bool V2>
__global__ __launch_bounds__(THREADS) void scatter_kernel(ScatterArgs A) {
    __shared__ __attribute__((aligned(16))) double panel_i[KP * LDW];
    __shared__ __attribute__((aligned(16))) double panel_j[KP * LDW];
    __shared__ unsigned long long kept_rows;
    const int t = threadIdx.x, cp = t & 31, rr = t >> 5;
    const int w = t >> 6, l = t & 63, g = l >> 4, c = l & 15;
    unsigned ti, tj;
    tile_of(blockIdx.x, A.tiles, ti, tj);
    const bool diag = ti == tj;
    const uint64_t slab = blockIdx.y, dim = A.dim;
    const uint64_t i0 = (uint64_t)ti * TILE, j0 = (uint64_t)tj * TILE;
    const uint64_t r0 = slab * A.slab_rows < A.n_rows ? slab * A.slab_rows : A.n_rows;
    const uint64_t r1 = r0 + A.slab_rows < A.n_rows ? r0 + A.slab_rows : A.n_rows;
    const uint64_t n_panels = (r1 - r0 + KP - 1) / KP;
    const bool count_here = blockIdx.x == 0 && A.st != nullptr;
    if (t == 0) kept_rows = 0;

    const uint64_t ci = i0 + 2 * cp, cj = j0 + 2 * cp;
    const bool oki0 = ci < dim, oki1 = ci + 1 < dim, okj0 = cj < dim, okj1 = cj + 1 < dim;
    const double ci0 = oki0 ? A.c[ci] : 0.0, ci1 = oki1 ? A.c[ci + 1] : 0.0, cj0 = okj0 ? A.c[cj] : 0.0, cj1 = okj1 ? A.c[cj + 1] : 0.0;
    double* const pj = diag ? panel_i : panel_j;

    // which of the thread's four rows of a panel are kept (bit u: row row0 + rr + 8 u)
    auto keep_of = [&](uint64_t row0) -> unsigned {
        unsigned k = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t r = row0 + (uint64_t)(rr + 8 * u);
            if (r < r1 && row_ok(A.st, r)) k |= 1u << u;
        }
        return k;
    };

    // the stripe of wavefront w: rows i0 + 16 w ..; 16 x 16 blocks jj_lo .. nj - 1 in accumulators 0 .. n_acc - 1 (a diagonal tile: from the
    // diagonal block on — the merge reads j >= i only); a stripe or a block wholly beyond dim is skipped
    const int nj = (int)((dim - j0 + 15) / 16 < 4 ? (dim - j0 + 15) / 16 : 4);
    const int jj_lo = diag ? w : 0, n_acc = nj - jj_lo;
    const bool stripe = i0 + 16u * (unsigned)w < dim && n_acc > 0;
    v4d acc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc[jj] = v4d{0.0, 0.0, 0.0, 0.0};

    double raw_i[8], raw_j[8];
    unsigned keep = 0;
    unsigned long long my_kept = 0;
    if (n_panels) {
        keep = keep_of(r0);
        fetch<V2>(A.x, dim, r0, keep, ci, rr, raw_i);
        if (!diag) fetch<V2>(A.x, dim, r0, keep, cj, rr, raw_j);
    }
    for (uint64_t p = 0; p < n_panels; ++p) {
        stage(panel_i, keep, oki0, oki1, ci0, ci1, rr, cp, raw_i);
        if (!diag) stage(panel_j, keep, okj0, okj1, cj0, cj1, rr, cp, raw_j);
        if (count_here && cp == 0) my_kept += (unsigned long long)__builtin_popcount(keep);
        __syncthreads();
        if (p + 1 < n_panels) {              // the next panel's rows travel while this one is multiplied
            const uint64_t row0 = r0 + (p + 1) * KP;
            keep = keep_of(row0);
            fetch<V2>(A.x, dim, row0, keep, ci, rr, raw_i);
            if (!diag) fetch<V2>(A.x, dim, row0, keep, cj, rr, raw_j);
        }
        if (stripe) {
            const double* ai = panel_i + g * LDW + 16 * w + c;
            const double* bj = pj + g * LDW + 16 * jj_lo + c;
            switch (n_acc) {             // (wave-uniform; a compile-time count keeps the accumulators where they are)
            case 4: mma_panel<4>(ai, bj, acc); break;
            case 3: mma_panel<3>(ai, bj, acc); break;
            case 2: mma_panel<2>(ai, bj, acc); break;
            default: mma_panel<1>(ai, bj, acc); break;
            }
        }
        __syncthreads();
    }
    // C/D layout of the f64 MFMA: lane (g, c) holds rows g + 4 r, r = 0 .. 3, of column c
    if (stripe) {
        double* out = A.partial + (slab * A.n_upper + blockIdx.x) * (uint64_t)(TILE * TILE);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n_acc) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(16 * w + g + 4 * r) * TILE + 16 * (jj_lo + q) + c] = acc[q][r];
            }
    }
    if (count_here) {
        if (n_panels == 0) __syncthreads();          // (kept_rows = 0 above must be visible; with panels the loop's barriers did that)
        if (cp == 0 && my_kept) atomicAdd(&kept_rows, my_kept);
        __syncthreads();
        if (t == 0) A.slab_count[slab] = (double)kept_rows;
    }
}

// grid (n_upper, 16): one thread per output of the macro tile; slab partials in slab order from +0.0, the result and its mirror
__global__ __launch_bounds__(THREADS) void scatter_merge_kernel(uint64_t n_slabs, uint64_t n_rows, uint64_t dim, unsigned tiles, unsigned n_upper,
                                                                const double* partial, const double* slab_count, int have_stats,
                                                                double* S, double* count) {
    unsigned ti, tj;
    tile_of(blockIdx.x, tiles, ti, tj);
    const unsigned e = blockIdx.y * THREADS + threadIdx.x, li = e >> 6, lj = e & 63;
    const uint64_t i = (uint64_t)ti * TILE + li, j = (uint64_t)tj * TILE + lj;
    if (i < dim && j < dim && (ti != tj || lj >= li)) {
        const double* p = partial + (uint64_t)blockIdx.x * (TILE * TILE) + e;
        double s = 0.0;
        for (uint64_t sl = 0; sl < n_slabs; ++sl) s = s + p[sl * n_upper * (uint64_t)(TILE * TILE)];
        S[i * dim + j] = s;
        if (i != j) S[j * dim + i] = s;
    }
    if (count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        double n = (double)n_rows;
        if (have_stats) {
            n = 0.0;
            for (uint64_t sl = 0; sl < n_slabs; ++sl) n = n + slab_count[sl];          // (integers below 2^53: exact in any order)
        }
        *count = n;
    }
}

nm_status pfail(nm_status st, const std::string& msg) { nm::pooled::set_error("nm_pooled_scatter: " + msg); return st; }
}  // namespace

// declared in include/nuts_amd.h
extern "C" nm_status nm_pooled_scatter(uint64_t n_rows, uint64_t dim, const double* d_rows, const double* d_center, const nm_draw_stats* d_stats,
                                       double* d_scatter, double* d_count, void* stream) {
    // ---- everything that can be refused is refused before the first device call
    if (!d_rows || !d_center || !d_scatter) return pfail(NM_ERR_INVALID_ARG, "null rows, center or scatter");
    if (n_rows == 0 || dim == 0) return pfail(NM_ERR_INVALID_ARG, "n_rows and dim must be positive");
    if (dim > NM_SCATTER_MAX_DIM) return pfail(NM_ERR_INVALID_ARG, "dim above NM_SCATTER_MAX_DIM (" + std::to_string(NM_SCATTER_MAX_DIM) + ")");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return pfail(NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    uint64_t n_slabs = (n_rows + NM_SCATTER_SLAB_MIN_ROWS - 1) / NM_SCATTER_SLAB_MIN_ROWS;
    n_slabs = n_slabs < 1 ? 1 : n_slabs > NM_SCATTER_MAX_SLABS ? NM_SCATTER_MAX_SLABS : n_slabs;
    const uint64_t per = (n_rows + n_slabs - 1) / n_slabs, R = 4 * ((per + 3) / 4);
    const unsigned T = (unsigned)((dim + TILE - 1) / TILE), n_upper = T * (T + 1) / 2;
    const uint64_t n_partial = n_slabs * n_upper * (uint64_t)(TILE * TILE);
    double* scratch = nullptr;
    hipError_t e = hipMallocAsync((void**)&scratch, (n_partial + n_slabs) * sizeof(double), s);
    if (e != hipSuccess) return pfail(NM_ERR_HIP, hipGetErrorString(e));
    ScatterArgs A;
    A.x = d_rows; A.c = d_center; A.st = d_stats; A.partial = scratch; A.slab_count = scratch + n_partial;
    A.n_rows = n_rows; A.dim = dim; A.slab_rows = R; A.tiles = T; A.n_upper = n_upper;
    const dim3 grid(n_upper, (unsigned)n_slabs);
    // 16 bytes per lane where every row starts 16-byte aligned, else 8
    if (dim % 2 == 0 && (reinterpret_cast<uintptr_t>(d_rows) & 15) == 0) hipLaunchKernelGGL(scatter_kernel<true>, grid, dim3(THREADS), 0, s, A);
    else hipLaunchKernelGGL(scatter_kernel<false>, grid, dim3(THREADS), 0, s, A);
    hipLaunchKernelGGL(scatter_merge_kernel, dim3(n_upper, TILE * TILE / THREADS), dim3(THREADS), 0, s, n_slabs, n_rows, dim, T, n_upper,
                       (const double*)scratch, (const double*)(scratch + n_partial), d_stats ? 1 : 0, d_scatter, d_count);
    e = hipGetLastError();
    (void)hipFreeAsync(scratch, s);
    if (e != hipSuccess) return pfail(NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}
