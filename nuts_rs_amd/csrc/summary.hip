// summary.hip — posterior summaries of a recorded trace on the device (nm_summarize_draws, include/nuts_amd.h): per element the mean,
// sd, within-series variance, split R-hat, ESS (Geyer's initial monotone sequence) and the chain-averaged autocorrelations.
// NOT reference behaviour: nutpie leaves summaries to ArviZ on the host; the definition is this repository's and the header
// states it operation by operation, so that tests/summary_ref.py restates it in numpy with the same bits.
//
// A post-pass over buffers the draw calls have written; engine-free like nm_pooled_partials, and no draw kernel is involved.
//   series kernel  one wavefront per (chunk of 32 series, tile of columns).  A lane owns V adjacent columns of a draw row (V = 2, one
//                  16-byte load per lane and row, up to 16 lags; 32 and 64 lags keep too many sums per lane for that); where a row is narrower than the wavefront, G series of the chunk sit side by side in
//                  it, so that the lanes still read one contiguous run of `chain * dim + d` (dim = 1: 32 chains, 256 B per row).
//                  Per series the column is read twice: once summed (the mean), once centred.  The last LCAP + 1 centred values live in
//                  an LDS ring [slot][lane]; the LCAP + 1 lag sums are registers (LCAP = 8 / 16 / 32 / 64, the smallest >= L; lags
//                  above L are computed and dropped).  Series results meet in LDS and lane group 0 adds them in series order
//                  to the chunk's partial sums.
//   merge kernel   chunk partials added in chunk order (one wavefront per row and tile of columns); run again on the squared deviations.
//   sqdev kernel   (mean_m - gm)^2 per chunk, serial in m — gm exists only after the merge.
//   finish kernel  one thread per column: sd, rhat, rho, ess, the flag.
// Every sum has ONE order whatever the grid: the same trace gives the same bits.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "../../include/nuts_amd.h"

namespace {
constexpr int CH = NM_SUMMARY_CHUNK_CHAINS;
constexpr int WAVE = 64;

struct SeriesArgs {
    const double* x;            // [N][C][D]
    const uint64_t* ids;        // device, [csel] or null
    double* means;              // [M][D]
    double* chain_var;          // [M][D] or null
    double* partial;            // [chunks][L + 3][D]: sum mean_m, sum var_m, sum acov_m[0 .. L]
    uint64_t row_stride;        // C * D
    uint64_t dim, csel, m_series, n, t_second;      // t_second: first draw of the second half
    int lags;                   // L
    int tile_vecs, groups;      // lanes (of V columns) per series in a block, series side by side
};

template <int V> struct Vec { double v[V]; };
template <int V> __device__ inline Vec<V> ld(const double* p);
template <> __device__ inline Vec<1> ld<1>(const double* p) { Vec<1> r; r.v[0] = *p; return r; }
template <> __device__ inline Vec<2> ld<2>(const double* p) { const double2 q = *reinterpret_cast<const double2*>(p); Vec<2> r; r.v[0] = q.x; r.v[1] = q.y; return r; }
template <int V> __device__ inline Vec<V> lds_ld(const double* p) { return ld<V>(p); }
template <int V> __device__ inline void lds_st(double* p, const Vec<V>& a);
template <> __device__ inline void lds_st<1>(double* p, const Vec<1>& a) { *p = a.v[0]; }
template <> __device__ inline void lds_st<2>(double* p, const Vec<2>& a) { *reinterpret_cast<double2*>(p) = make_double2(a.v[0], a.v[1]); }

// One time step of the centred pass: lag k multiplies y with the value k slots back in the lane's ring, then y enters the ring at
// `slot`.  The ring values are fetched in batches of eight, so that their LDS latencies overlap.  WARM (the first LCAP steps of a
// series): a lag sum only takes products of values that exist — a select, the steps stay branch-free.
template <int LCAP, int V, bool WARM>
__device__ inline void lag_step(double* lane_ring, int& slot, int t, const Vec<V>& y, double (&acc)[LCAP + 1][V]) {
    constexpr int R = LCAP + 1, B = 8, STRIDE = WAVE * V;
#pragma unroll
    for (int j = 0; j < V; ++j) acc[0][j] = acc[0][j] + y.v[j] * y.v[j];
    int idx = slot;
#pragma unroll
    for (int kb = 1; kb <= LCAP; kb += B) {
        Vec<V> r[B];
#pragma unroll
        for (int i = 0; i < B; ++i) {
            idx = idx == 0 ? R - 1 : idx - 1;
            r[i] = lds_ld<V>(lane_ring + idx * STRIDE);
        }
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double next = acc[kb + i][j] + y.v[j] * r[i].v[j];
                acc[kb + i][j] = (!WARM || kb + i <= t) ? next : acc[kb + i][j];          // (WARM: the slot may hold anything)
            }
    }
    lds_st<V>(lane_ring + slot * STRIDE, y);
    slot = slot + 1 == R ? 0 : slot + 1;
}
// Two steps t, t + 1 of the steady state on ONE pass over the ring: the value j slots back, y_{t-j}, serves lag j of step t and lag j + 1
// of step t + 1.  Lags run downwards, so that every lag sum still receives its terms in draw order (lag j + 1 has step t's term from
// the iteration before, lag 1 gets y_{t+1} y_t last).  Halves the LDS reads of the pass.
template <int LCAP, int V>
__device__ inline void lag_pair(double* lane_ring, int& slot, const Vec<V>& y0, const Vec<V>& y1, double (&acc)[LCAP + 1][V]) {
    constexpr int R = LCAP + 1, B = 8, STRIDE = WAVE * V;
    int idx = slot + 1 == R ? 0 : slot + 1;          // the oldest value: LCAP slots back
#pragma unroll
    for (int jb = LCAP; jb >= 1; jb -= B) {
        Vec<V> r[B];
#pragma unroll
        for (int i = 0; i < B; ++i) {
            r[i] = lds_ld<V>(lane_ring + idx * STRIDE);
            idx = idx + 1 == R ? 0 : idx + 1;
        }
#pragma unroll
        for (int i = 0; i < B; ++i) {
            const int lag = jb - i;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[lag][j] = acc[lag][j] + y0.v[j] * r[i].v[j];
                if (lag + 1 <= LCAP) acc[lag + 1][j] = acc[lag + 1][j] + y1.v[j] * r[i].v[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        acc[0][j] = acc[0][j] + y0.v[j] * y0.v[j];
        acc[1][j] = acc[1][j] + y1.v[j] * y0.v[j];
        acc[0][j] = acc[0][j] + y1.v[j] * y1.v[j];
    }
    lds_st<V>(lane_ring + slot * STRIDE, y0);
    slot = slot + 1 == R ? 0 : slot + 1;
    lds_st<V>(lane_ring + slot * STRIDE, y1);
    slot = slot + 1 == R ? 0 : slot + 1;
}

template <int LCAP, int V>
__global__ __launch_bounds__(WAVE) void summary_series_kernel(SeriesArgs A) {
    constexpr int ROWS = LCAP + 3, PF = 4;
    __shared__ __attribute__((aligned(16))) double ring[ROWS * WAVE * V];
    const int lane = threadIdx.x;
    double* const lane_ring = ring + lane * V;
    const int g = lane / A.tile_vecs, dv = lane - g * A.tile_vecs;
    const uint64_t d = ((uint64_t)blockIdx.x * A.tile_vecs + dv) * V;
    const bool col_ok = g < A.groups && d < A.dim;           // (V = 2: dim is even, so d + 1 < dim as well)
    const uint64_t chunk = blockIdx.y, m0 = chunk * CH;
    const int L = A.lags;
    const double nd = (double)A.n;
    for (int i0 = 0; i0 < CH && m0 + i0 < A.m_series; i0 += A.groups) {
        const uint64_t m = m0 + i0 + g;
        const bool ok = col_ok && i0 + g < CH && m < A.m_series;
        Vec<V> mean;
        double acc[LCAP + 1][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            mean.v[j] = 0.0;
#pragma unroll
            for (int k = 0; k <= LCAP; ++k) acc[k][j] = 0.0;
        }
        if (ok) {
            const uint64_t half = m / A.csel, cs = m - half * A.csel;
            const uint64_t chain = A.ids ? A.ids[cs] : cs;
            const double* p = A.x + (half ? A.t_second : 0) * A.row_stride + chain * A.dim + d;
            const uint64_t n = A.n, rs = A.row_stride;
            // pass 1: the mean, summed in draw order
            double sum[V];
#pragma unroll
            for (int j = 0; j < V; ++j) sum[j] = 0.0;
            uint64_t t = 0;
            for (; t + 8 <= n; t += 8) {
                Vec<V> q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = ld<V>(p + (t + u) * rs);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int j = 0; j < V; ++j) sum[j] = sum[j] + q[u].v[j];
            }
            for (; t < n; ++t) {
                const Vec<V> q = ld<V>(p + t * rs);
#pragma unroll
                for (int j = 0; j < V; ++j) sum[j] = sum[j] + q.v[j];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) mean.v[j] = sum[j] / nd;
            // pass 2: the lag sums of the centred column; the ring holds y_{t - LCAP} .. y_t
            // (the first LCAP draws in the guarded form; then pairs of draws; the next PF rows are in flight while PF are consumed)
            int slot = 0;
            Vec<V> cur[PF], nxt[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) { const uint64_t tt = (uint64_t)u < n ? u : n - 1; cur[u] = ld<V>(p + tt * rs); }
            for (t = 0; t < n; t += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) { const uint64_t tt = t + PF + u < n ? t + PF + u : n - 1; nxt[u] = ld<V>(p + tt * rs); }
                Vec<V> y[PF];
#pragma unroll
                for (int u = 0; u < PF; ++u)
#pragma unroll
                    for (int j = 0; j < V; ++j) y[u].v[j] = cur[u].v[j] - mean.v[j];
                if (t < (uint64_t)LCAP) {                 // (LCAP is a multiple of PF: the whole group is in the warm-up)
#pragma unroll
                    for (int u = 0; u < PF; ++u)
                        if (t + u < n) lag_step<LCAP, V, true>(lane_ring, slot, (int)t + u, y[u], acc);
                } else if (t + PF <= n) {
                    lag_pair<LCAP, V>(lane_ring, slot, y[0], y[1], acc);
                    lag_pair<LCAP, V>(lane_ring, slot, y[2], y[3], acc);
                } else {
#pragma unroll
                    for (int u = 0; u < PF; ++u)
                        if (t + u < n) lag_step<LCAP, V, false>(lane_ring, slot, 0, y[u], acc);
                }
#pragma unroll
                for (int u = 0; u < PF; ++u) cur[u] = nxt[u];
            }
        }
        // the series' results meet in LDS (the ring is free now): rows 0 mean, 1 var, 2 + k acov[k]
        __syncthreads();
        if (ok) {
            Vec<V> var;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[0][j] = acc[0][j] / nd;
                var.v[j] = acc[0][j] * nd / (nd - 1.0);
            }
#pragma unroll
            for (int k = 1; k <= LCAP; ++k)
#pragma unroll
                for (int j = 0; j < V; ++j) acc[k][j] = acc[k][j] / nd;
            lds_st<V>(ring + ((size_t)0 * WAVE + lane) * V, mean);
            lds_st<V>(ring + ((size_t)1 * WAVE + lane) * V, var);
#pragma unroll
            for (int k = 0; k <= LCAP; ++k) {
                Vec<V> a;
#pragma unroll
                for (int j = 0; j < V; ++j) a.v[j] = acc[k][j];
                lds_st<V>(ring + ((size_t)(2 + k) * WAVE + lane) * V, a);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                A.means[m * A.dim + d + j] = mean.v[j];
                if (A.chain_var) A.chain_var[m * A.dim + d + j] = var.v[j];
            }
        }
        __syncthreads();
        if (col_ok && g == 0) {
            // lane group 0 adds the round's series, in series order, to the chunk's partial sums (its own words of global memory, row by row: fetched
            // all at once they stay in registers beside the lag sums and the 32-lag kernel loses its second wavefront per SIMD)
            double* out = A.partial + chunk * (uint64_t)(L + 3) * A.dim + d;
            for (int row = 0; row < L + 3; ++row) {
                Vec<V> sum;
#pragma unroll
                for (int j = 0; j < V; ++j) sum.v[j] = i0 == 0 ? 0.0 : out[(uint64_t)row * A.dim + j];
                for (int gg = 0; gg < A.groups && i0 + gg < CH && m0 + i0 + gg < A.m_series; ++gg) {
                    const Vec<V> c = lds_ld<V>(ring + ((size_t)row * WAVE + gg * A.tile_vecs + dv) * V);
#pragma unroll
                    for (int j = 0; j < V; ++j) sum.v[j] = sum.v[j] + c.v[j];
                }
#pragma unroll
                for (int j = 0; j < V; ++j) out[(uint64_t)row * A.dim + j] = sum.v[j];
            }
        }
        __syncthreads();
    }
}

// grid (ceil(dim / dt), rows), one wavefront: totals[row][d] = the chunks' values in chunk order.  A lane (sub, dd) fetches column dd of
// chunks c0 + u * cs + sub, u = 0 .. 7 — `cs` chunks side by side where a row is narrower than the wavefront, eight loads in flight —,
// the values meet in LDS and the lanes of sub 0 add them in chunk order.
__global__ __launch_bounds__(WAVE) void summary_merge_kernel(uint64_t chunks, uint64_t rows, uint64_t dim, const double* partial, double* totals,
                                                            int dt, int cs) {
    __shared__ double buf[8][WAVE];
    const int lane = threadIdx.x, sub = lane / dt, dd = lane - sub * dt;
    const uint64_t d = (uint64_t)blockIdx.x * dt + dd, row = blockIdx.y;
    const bool ok = sub < cs && d < dim;
    double s = 0.0;
    for (uint64_t c0 = 0; c0 < chunks; c0 += 8 * (uint64_t)cs) {
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint64_t c = c0 + (uint64_t)u * cs + sub;
            q[u] = (ok && c < chunks) ? partial[(c * rows + row) * dim + d] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) buf[u][lane] = q[u];
        __syncthreads();
        if (ok && sub == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                for (int g = 0; g < cs; ++g)
                    if (c0 + (uint64_t)u * cs + g < chunks) s = s + buf[u][g * dt + dd];
        }
        __syncthreads();
    }
    if (ok && sub == 0) totals[row * dim + d] = s;
}
// grid (ceil(dim / 128), chunks): sq[chunk][d] = sum over the chunk's series, in series order, of (mean_m - gm)^2
__global__ __launch_bounds__(128) void summary_sqdev_kernel(uint64_t m_series, uint64_t dim, const double* means, const double* totals, double* sq) {
    const uint64_t d = (uint64_t)blockIdx.x * 128u + threadIdx.x, chunk = blockIdx.y;
    if (d >= dim) return;
    const double gm = totals[d] / (double)m_series;
    const uint64_t m0 = chunk * CH, m1 = m0 + CH < m_series ? m0 + CH : m_series;
    double s = 0.0;
    for (uint64_t m = m0; m < m1; ++m) {
        const double dl = means[m * dim + d] - gm;
        s = s + dl * dl;
    }
    sq[chunk * dim + d] = s;
}
// totals: rows 0 .. L + 2 as the partials, row L + 3 the summed squared deviations
__global__ __launch_bounds__(128) void summary_finish_kernel(uint64_t m_series, uint64_t n, int L, uint64_t dim, const double* totals, nm_summary_outputs o) {
    const uint64_t d = (uint64_t)blockIdx.x * 128u + threadIdx.x;
    if (d >= dim) return;
    const double md = (double)m_series, nd = (double)n;
    const double ssq = totals[(uint64_t)(L + 3) * dim + d];
    const double gm = totals[d] / md, w = totals[dim + d] / md, bn = ssq / (md - 1.0);
    const double var_plus = w * (nd - 1.0) / nd + bn;
    auto rho = [&](int k) -> double {
        if (k == 0) return 1.0;
        const double acov = totals[(uint64_t)(2 + k) * dim + d] / md;
        return 1.0 - (w - acov) / var_plus;
    };
    if (o.d_mean) o.d_mean[d] = gm;
    if (o.d_sd) o.d_sd[d] = sqrt(var_plus);
    if (o.d_within_var) o.d_within_var[d] = w;
    if (o.d_rhat) o.d_rhat[d] = sqrt(var_plus / w);
    if (o.d_autocorr)
        for (int k = 0; k <= L; ++k) o.d_autocorr[(uint64_t)k * dim + d] = rho(k);
    if (o.d_ess || o.d_ess_truncated) {
        const double p0 = rho(0) + rho(1);
        double tau = -1.0 + 2.0 * p0, prev = p0;
        uint64_t truncated = 1;
        for (int t = 1; 2 * t + 1 <= L; ++t) {
            const double pt = rho(2 * t) + rho(2 * t + 1);
            if (!(pt > 0.0)) { truncated = 0; break; }
            const double pm = pt < prev ? pt : prev;
            prev = pm;
            tau = tau + 2.0 * pm;
        }
        if (o.d_ess) o.d_ess[d] = (md * nd) / tau;
        if (o.d_ess_truncated) static_cast<uint64_t*>(o.d_ess_truncated)[d] = truncated;
    }
}

thread_local std::string g_serr;
nm_status sfail(nm_status st, const std::string& msg) { g_serr = "nm_summarize_draws: " + msg; return st; }

template <int V>
void launch_series(int lcap, dim3 grid, hipStream_t s, const SeriesArgs& A) {
    switch (lcap) {
    case 8: hipLaunchKernelGGL((summary_series_kernel<8, V>), grid, dim3(WAVE), 0, s, A); break;
    case 16: hipLaunchKernelGGL((summary_series_kernel<16, V>), grid, dim3(WAVE), 0, s, A); break;
    default:          // 2 x 33 lag sums per lane and the ring values in flight do not fit 256 registers: 32 and 64 lags run on 8-byte lanes
        if constexpr (V == 1) {
            if (lcap == 32) hipLaunchKernelGGL((summary_series_kernel<32, 1>), grid, dim3(WAVE), 0, s, A);
            else hipLaunchKernelGGL((summary_series_kernel<64, 1>), grid, dim3(WAVE), 0, s, A);
        }
        break;
    }
}
}  // namespace

extern "C" const char* nm_summary_last_error(void) { return g_serr.c_str(); }

extern "C" nm_status nm_summarize_draws(const nm_summary_spec* spec, const double* d_draws, const nm_summary_outputs* out, void* stream) {
    // ---- everything that can be refused is refused before the first device call
    if (!spec || !d_draws || !out) return sfail(NM_ERR_INVALID_ARG, "null spec, draws or outputs");
    const uint64_t N = spec->n_draws, C = spec->n_chains, D = spec->dim;
    if (N == 0 || C == 0 || D == 0) return sfail(NM_ERR_INVALID_ARG, "n_draws, n_chains and dim must be positive");
    if (spec->max_lag < 1 || spec->max_lag > 64) return sfail(NM_ERR_INVALID_ARG, "max_lag must be 1 .. 64");
    if (spec->split > 1) return sfail(NM_ERR_INVALID_ARG, "split must be 0 or 1");
    uint64_t csel = C;
    const uint64_t* h_ids = static_cast<const uint64_t*>(spec->h_chain_ids);
    if (h_ids) {
        csel = spec->n_chain_ids;
        for (uint64_t i = 0; i < csel; ++i) {
            if (h_ids[i] >= C) return sfail(NM_ERR_INVALID_ARG, "chain id out of range");
            if (i && h_ids[i] <= h_ids[i - 1]) return sfail(NM_ERR_INVALID_ARG, "chain ids must be strictly increasing");
        }
    }
    const uint64_t n = spec->split ? N / 2 : N, M = spec->split ? 2 * csel : csel;
    if (n < 2) return sfail(NM_ERR_INVALID_ARG, "fewer than 2 draws per series");
    if (M < 2) return sfail(NM_ERR_INVALID_ARG, "fewer than 2 series");
    const int L = (int)(spec->max_lag < n - 1 ? spec->max_lag : n - 1);
    const uint64_t chunks = (M + CH - 1) / CH, rows = (uint64_t)L + 3;
    if (chunks > 65535) return sfail(NM_ERR_INVALID_ARG, "more than 65535 chunks of 32 series");
    if ((D + 127) / 128 > 0x7fffffffull) return sfail(NM_ERR_INVALID_ARG, "dim above 128 * (2^31 - 1)");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sfail(NM_ERR_NO_DEVICE, "no HIP device available; there is no CPU fallback");
    hipStream_t s = (hipStream_t)stream;
    // scratch: partial [chunks][L + 3][D], sq [chunks][D], totals [L + 4][D], (means [M][D]), (ids [csel] as 8-byte words)
    const bool own_means = !out->d_chain_mean;
    const uint64_t n_partial = chunks * rows * D, n_sq = chunks * D, n_tot = (rows + 1) * D, n_means = own_means ? M * D : 0;
    const uint64_t n_ids = h_ids ? csel : 0;
    double* scratch = nullptr;
    hipError_t e = hipMallocAsync((void**)&scratch, (n_partial + n_sq + n_tot + n_means + n_ids) * sizeof(double), s);
    if (e != hipSuccess) return sfail(NM_ERR_HIP, hipGetErrorString(e));
    double *partial = scratch, *sq = partial + n_partial, *totals = sq + n_sq, *means = own_means ? totals + n_tot : out->d_chain_mean;
    uint64_t* d_ids = nullptr;
    if (n_ids) {
        d_ids = reinterpret_cast<uint64_t*>(totals + n_tot + n_means);
        e = hipMemcpyAsync(d_ids, h_ids, n_ids * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);          // the caller's array is free on return
        if (e != hipSuccess) { (void)hipFreeAsync(scratch, s); return sfail(NM_ERR_HIP, hipGetErrorString(e)); }
    }
    const int lcap = L <= 8 ? 8 : L <= 16 ? 16 : L <= 32 ? 32 : 64;
    // 16 bytes per lane where every row of every chain starts 16-byte aligned and the lag sums of two columns fit the registers
    const int V = (lcap <= 16 && D % 2 == 0 && (reinterpret_cast<uintptr_t>(d_draws) & 15) == 0) ? 2 : 1;
    const uint64_t dvecs = D / V;
    SeriesArgs A;
    A.x = d_draws; A.ids = d_ids; A.means = means; A.chain_var = out->d_chain_var; A.partial = partial;
    A.row_stride = C * D; A.dim = D; A.csel = csel; A.m_series = M; A.n = n; A.t_second = N - n; A.lags = L;
    uint64_t tiles;
    if (dvecs >= WAVE) {
        tiles = (dvecs + WAVE - 1) / WAVE;
        A.tile_vecs = (int)((dvecs + tiles - 1) / tiles);
        A.groups = 1;
    } else {
        tiles = 1;
        A.tile_vecs = (int)dvecs;
        A.groups = (int)(WAVE / dvecs) < CH ? (int)(WAVE / dvecs) : CH;
    }
    const dim3 grid((unsigned)tiles, (unsigned)chunks);
    if (V == 2) launch_series<2>(lcap, grid, s, A); else launch_series<1>(lcap, grid, s, A);
    const unsigned dblocks = (unsigned)((D + 127) / 128);
    const int dt = D < WAVE ? (int)D : WAVE, cs = WAVE / dt;
    const unsigned mblocks = (unsigned)((D + dt - 1) / dt);
    hipLaunchKernelGGL(summary_merge_kernel, dim3(mblocks, (unsigned)rows), dim3(WAVE), 0, s, chunks, rows, D, (const double*)partial, totals, dt, cs);
    hipLaunchKernelGGL(summary_sqdev_kernel, dim3(dblocks, (unsigned)chunks), dim3(128), 0, s, M, D, (const double*)means, (const double*)totals, sq);
    hipLaunchKernelGGL(summary_merge_kernel, dim3(mblocks, 1), dim3(WAVE), 0, s, chunks, (uint64_t)1, D, (const double*)sq, totals + rows * D, dt, cs);
    hipLaunchKernelGGL(summary_finish_kernel, dim3(dblocks), dim3(128), 0, s, M, n, L, D, (const double*)totals, *out);
    e = hipGetLastError();
    (void)hipFreeAsync(scratch, s);
    if (e != hipSuccess) return sfail(NM_ERR_HIP, hipGetErrorString(e));
    return NM_OK;
}
