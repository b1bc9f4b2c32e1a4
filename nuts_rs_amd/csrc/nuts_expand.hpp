// nuts_expand.hpp — `expand_vector` for device densities (reference CpuLogpFunc::expand_vector, src/math/cpu_math.rs:892-899, called by
// Chain::expanded_draw, src/chain.rs:201): the map from the unconstrained point the sampler moves to what the user reads, as ONE streaming
// kernel over recorded positions, [n_rows][dim] -> [n_rows][edim].  It is a pass after the draw launches, not a part of them: the draw
// kernels sit at their register caps, and one pass serves every kernel family (DESIGN "Expanded draws").
//
// A density takes part by defining the two optional members has_expand detects (nuts_kernels.hpp); element j of a row's expansion is a
// function of (params, row, j) alone, so the result does not depend on how threads are mapped to rows.  The chain's random stream is not
// available here (the reference hands expand_vector the generator; no density it ships uses it).
//
// Shape (a bandwidth kernel): a block of 256 threads takes a tile of whole rows, reads it flat — 16 B per lane from the first 16-byte
// boundary on, every load of the tile in flight before the first LDS write — into LDS, then produces the tile's outputs flat, two
// consecutive elements per lane, stored as 16 B where the output is aligned.  Rows longer than the LDS tile are read from global memory
// by the functor itself, one chunk of a row's outputs per block.  Blocks stride over the tiles; the grid is bounded by the caller.
#pragma once
#include <hip/hip_runtime.h>
#include "nuts_contract.hpp"
#include "nuts_kernels.hpp"

namespace nm {

constexpr int EXP_THREADS = 256;
constexpr int EXP_TILE = 2048;                    // doubles of positions a block keeps in LDS (16 KiB: eight blocks per CU)
constexpr int EXP_OUT_TILE = 4096;                // outputs of a tile, at most (unless one row has more)
constexpr int EXP_LOADS = EXP_TILE / (2 * EXP_THREADS);
constexpr int EXP_WIDE_CHUNK = 4 * EXP_THREADS;   // outputs per block and step of a row that does not fit the LDS tile

// rows per LDS tile (0: the rows do not fit, the functor reads global memory); shared by the kernel and its launcher
__host__ __device__ inline uint64_t expand_rows_per_tile(uint64_t dim, uint64_t edim) {
    if (dim > (uint64_t)EXP_TILE) return 0;
    const uint64_t by_in = (uint64_t)EXP_TILE / dim, by_out = (uint64_t)EXP_OUT_TILE / edim;
    const uint64_t r = by_in < by_out ? by_in : by_out;
    return r ? r : 1;
}

template <class Dens>
__global__ __launch_bounds__(EXP_THREADS) void nm_expand_kernel(const double* __restrict__ params, int dim, int edim, uint64_t n_rows,
                                                                const double* __restrict__ pos, double* __restrict__ out) {
    alignas(16) __shared__ double rows[EXP_TILE];
    dm_init_lds();                                  // the special functions' tables (an expansion may call nm::xexp / xlog)
    const int t = (int)threadIdx.x;
    const uint64_t R = expand_rows_per_tile((uint64_t)dim, (uint64_t)edim);
    if (R == 0) {
        // a row longer than the tile: work items are (row, chunk of EXP_WIDE_CHUNK outputs); x points to global memory
        const uint64_t chunks = ((uint64_t)edim + EXP_WIDE_CHUNK - 1) / EXP_WIDE_CHUNK;
        for (uint64_t w = blockIdx.x; w < n_rows * chunks; w += gridDim.x) {
            const uint64_t row = w / chunks;
            const int j0 = (int)(w - row * chunks) * EXP_WIDE_CHUNK;
            const double* x = pos + row * (uint64_t)dim;
            double* o = out + row * (uint64_t)edim;
#pragma unroll
            for (int u = 0; u < EXP_WIDE_CHUNK / EXP_THREADS; ++u) {
                const int j = j0 + u * EXP_THREADS + t;
                if (j < edim) o[j] = Dens::expand_element(params, dim, x, j);
            }
        }
        return;
    }
    const uint64_t n_tiles = (n_rows + R - 1) / R;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t row0 = tile * R;
        const int nr = (int)(n_rows - row0 < R ? n_rows - row0 : R);
        // ---- read nr * dim <= EXP_TILE doubles, flat: one leading double up to the 16-byte boundary, pairs, one trailing double
        const double* src = pos + row0 * (uint64_t)dim;
        const int n = nr * dim;
        int head = (int)((reinterpret_cast<uintptr_t>(src) >> 3) & 1);
        if (head > n) head = n;
        const int nb = (n - head) >> 1;
        const double2* body = reinterpret_cast<const double2*>(src + head);
        double2 q[EXP_LOADS];
#pragma unroll
        for (int u = 0; u < EXP_LOADS; ++u) {
            const int i = t + u * EXP_THREADS;
            q[u] = i < nb ? body[i] : make_double2(0.0, 0.0);
        }
        if (t < head) rows[t] = src[t];
        if (t == 0 && head + 2 * nb < n) rows[n - 1] = src[n - 1];
#pragma unroll
        for (int u = 0; u < EXP_LOADS; ++u) {
            const int i = t + u * EXP_THREADS;
            if (i < nb) { rows[head + 2 * i] = q[u].x; rows[head + 2 * i + 1] = q[u].y; }
        }
        __syncthreads();
        // ---- nr * edim outputs, flat: element o of the tile is (row o / edim, j = o mod edim)
        double* dst = out + row0 * (uint64_t)edim;
        const int m = nr * edim;
        int ohead = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
        if (ohead > m) ohead = m;
        const int mb = (m - ohead) >> 1;
        auto element = [&](int o) { const int r = o / edim; return Dens::expand_element(params, dim, rows + r * dim, o - r * edim); };
        if (t < ohead) dst[t] = element(t);
        if (t == 0 && ohead + 2 * mb < m) dst[m - 1] = element(m - 1);
        double2* obody = reinterpret_cast<double2*>(dst + ohead);
        for (int i = t; i < mb; i += EXP_THREADS) {
            const int o = ohead + 2 * i;
            obody[i] = make_double2(element(o), element(o + 1));
        }
        __syncthreads();                            // the next tile overwrites `rows`
    }
}

// Enqueue the expansion of n_rows rows on `stream`.  grid_cap: blocks in the grid at most (0: eight per compute unit of the current device).
// A density without the two members has no kernel: its expansion is the identity, which the caller serves with a copy.
template <class Dens>
inline hipError_t launch_expand_t(const double* d_params, uint64_t dim, uint64_t edim, uint64_t n_rows, const double* d_positions,
                                  double* d_expanded, unsigned grid_cap, hipStream_t stream) {
    if constexpr (has_expand<Dens>::value) {
        if (n_rows == 0 || edim == 0) return hipSuccess;
        if (dim == 0 || dim > 0x3fffffffull || edim > 0x3fffffffull) return hipErrorInvalidValue;      // (the kernel indexes with int)
        const uint64_t R = expand_rows_per_tile(dim, edim);
        const uint64_t items = R ? (n_rows + R - 1) / R : n_rows * ((edim + EXP_WIDE_CHUNK - 1) / EXP_WIDE_CHUNK);
        uint64_t cap = grid_cap;
        if (!cap) {
            int dev = 0, cus = 0;
            hipError_t er = hipGetDevice(&dev);
            if (er == hipSuccess) er = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            if (er != hipSuccess) return er;
            cap = 8ull * (uint64_t)(cus > 0 ? cus : 1);
        }
        const unsigned grid = (unsigned)(items < cap ? items : cap);
        hipLaunchKernelGGL((nm_expand_kernel<Dens>), dim3(grid), dim3(EXP_THREADS), 0, stream, d_params, (int)dim, (int)edim, n_rows, d_positions, d_expanded);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

}  // namespace nm
