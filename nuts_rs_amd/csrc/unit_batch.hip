// unit_batch.hip — the unit-parity surface of libnuts_amd.so: single pieces of the kernels' arithmetic (one leapfrog, the maps of the
// low-rank transformation, a U-turn test, the special functions, the ziggurat) on batches of rows, so that tests can compare each with
// the oracle's.  The only host-side unit that instantiates the chain kernels' device code (next to math_seam.hip, the scalar seam).
#include <cstring>
#include <vector>
#include "nuts_launch.hpp"
#include "engine_host.hpp"
using namespace nm;
using namespace nm::host;
// ---------------------------------------------------------------------------------------------
// batched Math primitives (unit-parity surface): rows are [n][dim], unpadded
// ---------------------------------------------------------------------------------------------
namespace nm {
struct LfArgs {
    KParams P;
    const double *z, *v, *gz, *sigma, *mu, *eps, *logdet, *e0;
    double *z_out, *v_out, *gz_out, *x_out, *gx_out, *logp_out, *ke_out, *err_out;
};
template <int DPL>
NM_DEV void load_row(Tile<DPL>& t, const double* row, int dim) {
#pragma unroll
    for (int k = 0; k < DPL; ++k) { int d = elem_index<1>(k); t.a[k] = d < dim ? row[d] : 0.0; }
}
template <int DPL>
NM_DEV void store_row(const Tile<DPL>& t, double* row, int dim) {
#pragma unroll
    for (int k = 0; k < DPL; ++k) { int d = elem_index<1>(k); if (d < dim) row[d] = t.a[k]; }
}
template <int DPL, class Dens>
__global__ __launch_bounds__(64) void leapfrog_batch_kernel(const LfArgs A) {
    dm_init_lds();
    const uint64_t i = blockIdx.x;
    const int dim = (int)A.P.dim;
    __shared__ double lsig[64 * DPL], lmu[64 * DPL], lred[2 * RED_MAX_VALUES];
    __shared__ ChainScalars lsc;
    __shared__ double ldens[Dens::kNeedsLdsVector ? 64 * DPL : 2];
    ChainCtx<DPL, 1, Dens> C(A.P, lsc);
    C.dim = dim;
    C.red.init(lred);
    C.dens.init(A.P.logp_params, dim, C.red);
    C.dens.set_lds(ldens);
    C.lsig = lsig; C.lmu = lmu;
    {
        Tile<DPL> t;
        load_row(t, A.sigma + i * dim, dim); C.store(t, C.lsig);
        load_row(t, A.mu + i * dim, dim); C.store(t, C.lmu);
    }
    Pt<DPL> s0, s;
    load_row(s0.z, A.z + i * dim, dim);
    load_row(s0.v, A.v + i * dim, dim);
    load_row(s0.g, A.gz + i * dim, dim);
    Tile<DPL> x, gx;
    leapfrog(C, s0, s, A.eps[i], &x, &gx);
    store_row(s.z, A.z_out + i * dim, dim); store_row(s.v, A.v_out + i * dim, dim);
    store_row(s.g, A.gz_out + i * dim, dim); store_row(x, A.x_out + i * dim, dim);
    store_row(gx, A.gx_out + i * dim, dim);
    if (lane_id() == 0) {
        A.logp_out[i] = s.logp;
        A.ke_out[i] = s.ke;
        A.err_out[i] = (s.ke - (s.logp + A.logdet[i])) - A.e0[i];
    }
}
// the three maps of the low-rank transformation for chain i of a batch (nm_lowrank_transform_batch): the block first
// packs its chain's unpadded inputs into the engine's layouts (pvec slots, lrvec rows, lrval), then applies the map
struct LrtArgs {
    KParams P;
    uint64_t which, n_eig;
    const double *stds, *mean, *vals, *vecs, *mu_lr, *in;
    double* out;
};
template <int DPL>
__global__ __launch_bounds__(64) void lowrank_transform_batch_kernel(const LrtArgs A) {
    dm_init_lds();
    typedef LrWrap<IidNormal> D;
    const uint64_t i = blockIdx.x;
    const int dim = (int)A.P.dim;
    __shared__ double lsig[64 * DPL], lmu[64 * DPL], lred[2 * RED_MAX_VALUES];
    __shared__ ChainScalars lsc;
    ChainCtx<DPL, 1, D> C(A.P, lsc);
    C.dim = dim;
    C.red.init(lred);
    C.lsig = lsig; C.lmu = lmu;
    C.slot_bytes = (int)(A.P.dpad * 8);
    C.voff = tid() * 16;
    C.pv = A.P.pvec + (size_t)i * NUM_PSLOT * A.P.dpad;
    C.rp = make_rsrc(C.pv, (uint64_t)NUM_PSLOT * A.P.dpad * 8);
    double* lv = A.P.lrvec + (size_t)i * (1 + A.P.lr_rmax) * A.P.dpad;
    double* lw = A.P.lrval + (size_t)i * 2 * A.P.lr_rmax;
    C.rl = make_rsrc(lv, (uint64_t)(1 + A.P.lr_rmax) * A.P.dpad * 8);
    C.lvals = lw;
    Tile<DPL> t, u;
    load_row(t, A.stds + i * dim, dim); C.store(t, C.lsig);
#pragma unroll
    for (int k = 0; k < DPL; ++k) u.a[k] = elem_index<1>(k) < dim ? 1.0 / t.a[k] : 0.0;
    C.storeP(u, P_ISIG);
    load_row(t, A.mean + i * dim, dim); C.store(t, C.lmu);
    load_row(t, A.mu_lr + i * dim, dim); C.store(t, lv);
    for (uint64_t k = 0; k < A.n_eig; ++k) {
        load_row(t, A.vecs + (i * A.n_eig + k) * dim, dim);
        C.store(t, lv + (1 + k) * A.P.dpad);
    }
    for (uint64_t k = tid(); k < A.n_eig; k += 64) {
        const double sq = __builtin_sqrt(A.vals[i * A.n_eig + k]);
        lw[k] = sq; lw[A.P.lr_rmax + k] = 1.0 / sq;
    }
    if (tid() == 0) { lsc.lr_has_inner = 1; lsc.lr_rank = A.n_eig; }
    __threadfence_block();
    __syncthreads();
    load_row(t, A.in + i * dim, dim);
    if (A.which == 0) transform_to_z(C, t, u);
    else if (A.which == 1) transform_to_x(C, t, u);
    else transform_to_gz(C, t, u);
    store_row(u, A.out + i * dim, dim);
}

template <int DPL>
__global__ __launch_bounds__(64) void turning_batch_kernel(uint64_t dim, const double* zs, const double* vs,
                                                           const double* ze, const double* ve, double* out) {
    const uint64_t i = blockIdx.x;
    Tile<DPL> a, b, c, d;
    load_row(a, zs + i * dim, (int)dim); load_row(b, vs + i * dim, (int)dim);
    load_row(c, ze + i * dim, (int)dim); load_row(d, ve + i * dim, (int)dim);
    double t1 = 0., t2 = 0.;
#pragma unroll
    for (int k = 0; k < DPL; ++k) turn_acc(a.a[k], b.a[k], c.a[k], d.a[k], t1, t2);
    wave_sum2(t1, t2);
    if (lane_id() == 0) { out[2 * i] = t1; out[2 * i + 1] = t2; }
}
__global__ void scalar_math_kernel(uint64_t op, uint64_t n, const double* a, const double* b, double* out) {
    dm_init_lds();
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], y = b ? b[i] : 0.0, r;
    switch (op) {
    case 0: r = dexp(x); break;
    case 1: r = dlog(x); break;
    case 2: r = dlog1p(x); break;
    case 3: r = logaddexp_lane(x, y); break;
    case 4: r = __builtin_sqrt(x); break;
    case 5: r = x / y; break;
    case 7: r = dexpm1(x); break;
    case 8: r = dsincos(x).x; break;
    case 9: r = dsincos(x).y; break;
    default: r = __builtin_nan("");
    }
    out[i] = r;
}
__global__ __launch_bounds__(64) void normal_batch_kernel(uint64_t count, const uint32_t* keys, const double* zig_x,
                                                          const double* zig_f, double* out, uint64_t* words) {
    dm_init_lds();
    __shared__ uint32_t cache[RNG_CACHE_WORDS];
    __shared__ double stage[1024];   // LDS staging in this test kernel (the engine stages through its HBM scratch)
    const uint64_t i = blockIdx.x;
    DevRng rng;
    rng.init(keys + 8 * i, 0, cache);
    ZigTables T = {zig_x, zig_f};
    uint64_t done = 0;
    while (done < count) {
        int chunk = (count - done) < 1024 ? (int)(count - done) : 1024;
        fill_standard_normals(rng, stage, chunk, T);
        for (int j = lane_id(); j < chunk; j += 64) out[i * count + done + j] = stage[j];
        __syncthreads();
        done += chunk;
    }
    if (words && lane_id() == 0) words[i] = rng.pos;
}
}  // namespace nm

template <class Dens>
static hipError_t launch_lf_d(int dpl, const LfArgs& A, uint64_t n, hipStream_t st) {
    dim3 g((unsigned)n), b(64);
    switch (dpl) {
    case 2: hipLaunchKernelGGL((leapfrog_batch_kernel<2, Dens>), g, b, 0, st, A); break;
    case 4: hipLaunchKernelGGL((leapfrog_batch_kernel<4, Dens>), g, b, 0, st, A); break;
    case 8: hipLaunchKernelGGL((leapfrog_batch_kernel<8, Dens>), g, b, 0, st, A); break;
    case 16: hipLaunchKernelGGL((leapfrog_batch_kernel<16, Dens>), g, b, 0, st, A); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" nm_status nm_leapfrog_batch(const nm_logp_spec* logp, uint64_t n, uint64_t dims_per_lane,
                                       const double* d_z, const double* d_v, const double* d_gz,
                                       const double* d_sigma, const double* d_mu,
                                       const double* d_eps, const double* d_logdet, const double* d_initial_energy,
                                       double* d_z_out, double* d_v_out, double* d_gz_out,
                                       double* d_x_out, double* d_gx_out,
                                       double* d_logp_out, double* d_kinetic_out, double* d_energy_error_out,
                                       void* stream) {
    nm_status st = check_logp(logp);
    if (st == NM_OK && (logp->kind == NM_LOGP_MODULE || logp->kind == NM_LOGP_HOST_CALLBACK)) return fail(NM_ERR_UNSUPPORTED, "nm_leapfrog_batch covers the built-in densities only");
    if (st != NM_OK) return st;
    st = ensure_device(-1);
    if (st != NM_OK) return st;
    const int dpl = pick_dpl(logp->dim, dims_per_lane);
    if (!dpl) return fail(NM_ERR_UNSUPPORTED, "unsupported dim / dims_per_lane");
    if (n == 0) return NM_OK;
    double* d_params = nullptr;
    HIP_TRY(hipMalloc(&d_params, (logp->n_params ? logp->n_params : 1) * sizeof(double)));
    if (logp->n_params) HIP_TRY(copy_on((hipStream_t)stream, d_params, logp->h_params, logp->n_params * sizeof(double), hipMemcpyHostToDevice));
    LfArgs A;
    memset(&A, 0, sizeof A);
    A.P.dim = logp->dim; A.P.dpad = 64ull * dpl; A.P.logp_params = d_params; A.P.n_chains = n;
    A.z = d_z; A.v = d_v; A.gz = d_gz; A.sigma = d_sigma; A.mu = d_mu; A.eps = d_eps; A.logdet = d_logdet; A.e0 = d_initial_energy;
    A.z_out = d_z_out; A.v_out = d_v_out; A.gz_out = d_gz_out; A.x_out = d_x_out; A.gx_out = d_gx_out;
    A.logp_out = d_logp_out; A.ke_out = d_kinetic_out; A.err_out = d_energy_error_out;
    hipError_t er;
    switch (logp->kind) {
    case NM_LOGP_IID_NORMAL: er = launch_lf_d<IidNormal>(dpl, A, n, (hipStream_t)stream); break;
    case NM_LOGP_DIAG_NORMAL: er = launch_lf_d<DiagNormal>(dpl, A, n, (hipStream_t)stream); break;
    case NM_LOGP_FUNNEL: er = launch_lf_d<Funnel>(dpl, A, n, (hipStream_t)stream); break;
    case NM_LOGP_MVN_PREC: er = launch_lf_d<MvnPrec>(dpl, A, n, (hipStream_t)stream); break;
    default: er = launch_lf_d<EightSchools>(2, A, n, (hipStream_t)stream); break;
    }
    if (er == hipSuccess) er = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d_params);
    if (er != hipSuccess) return fail(NM_ERR_HIP, "leapfrog_batch: %s", hipGetErrorString(er));
    return NM_OK;
}

extern "C" nm_status nm_lowrank_transform_batch(uint64_t which, uint64_t n, uint64_t dim, uint64_t n_eig, uint64_t dims_per_lane,
                                                const double* d_stds, const double* d_mean, const double* d_vals, const double* d_vecs,
                                                const double* d_mu_lr, const double* d_in, double* d_out, void* stream) {
    nm_status st = ensure_device(-1);
    if (st != NM_OK) return st;
    if (which > 2) return fail(NM_ERR_INVALID_ARG, "which must be 0 (x -> z), 1 (z -> x) or 2 (g_x -> g_z)");
    const int dpl = pick_dpl(dim, dims_per_lane);
    if (!dpl) return fail(NM_ERR_UNSUPPORTED, "unsupported dim / dims_per_lane (one wavefront per chain: dim <= 1024)");
    if (n == 0) return NM_OK;
    LrtArgs A;
    memset(&A, 0, sizeof A);
    const uint64_t dpad = 64ull * dpl, R = n_eig ? n_eig : 1;
    double *pv = nullptr, *lv = nullptr, *lw = nullptr;
    HIP_TRY(hipMalloc(&pv, n * NUM_PSLOT * dpad * 8));
    HIP_TRY(hipMalloc(&lv, n * (1 + R) * dpad * 8));
    HIP_TRY(hipMalloc(&lw, n * 2 * R * 8));
    A.P.dim = dim; A.P.dpad = dpad; A.P.n_chains = n; A.P.pvec = pv; A.P.lrvec = lv; A.P.lrval = lw; A.P.lr_rmax = R;
    A.which = which; A.n_eig = n_eig; A.stds = d_stds; A.mean = d_mean; A.vals = d_vals; A.vecs = d_vecs; A.mu_lr = d_mu_lr;
    A.in = d_in; A.out = d_out;
    dim3 g((unsigned)n), b(64);
    hipStream_t s = (hipStream_t)stream;
    hipError_t er = hipMemsetAsync(pv, 0, n * NUM_PSLOT * dpad * 8, s);
    if (er == hipSuccess) er = hipMemsetAsync(lv, 0, n * (1 + R) * dpad * 8, s);
    if (er == hipSuccess) {
        switch (dpl) {
        case 2: hipLaunchKernelGGL((lowrank_transform_batch_kernel<2>), g, b, 0, s, A); break;
        case 4: hipLaunchKernelGGL((lowrank_transform_batch_kernel<4>), g, b, 0, s, A); break;
        case 8: hipLaunchKernelGGL((lowrank_transform_batch_kernel<8>), g, b, 0, s, A); break;
        case 16: hipLaunchKernelGGL((lowrank_transform_batch_kernel<16>), g, b, 0, s, A); break;
        }
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    (void)hipFree(pv); (void)hipFree(lv); (void)hipFree(lw);
    if (er != hipSuccess) return fail(NM_ERR_HIP, "lowrank_transform_batch: %s", hipGetErrorString(er));
    return NM_OK;
}

extern "C" nm_status nm_turning_batch(uint64_t n, uint64_t dim, uint64_t dims_per_lane,
                                      const double* d_z_start, const double* d_v_start,
                                      const double* d_z_end, const double* d_v_end, double* d_out_t, void* stream) {
    nm_status st = ensure_device(-1);
    if (st != NM_OK) return st;
    const int dpl = pick_dpl(dim, dims_per_lane);
    if (!dpl) return fail(NM_ERR_UNSUPPORTED, "unsupported dim / dims_per_lane");
    if (n == 0) return NM_OK;
    dim3 g((unsigned)n), b(64);
    hipStream_t s = (hipStream_t)stream;
    switch (dpl) {
    case 2: hipLaunchKernelGGL((turning_batch_kernel<2>), g, b, 0, s, dim, d_z_start, d_v_start, d_z_end, d_v_end, d_out_t); break;
    case 4: hipLaunchKernelGGL((turning_batch_kernel<4>), g, b, 0, s, dim, d_z_start, d_v_start, d_z_end, d_v_end, d_out_t); break;
    case 8: hipLaunchKernelGGL((turning_batch_kernel<8>), g, b, 0, s, dim, d_z_start, d_v_start, d_z_end, d_v_end, d_out_t); break;
    case 16: hipLaunchKernelGGL((turning_batch_kernel<16>), g, b, 0, s, dim, d_z_start, d_v_start, d_z_end, d_v_end, d_out_t); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return NM_OK;
}

extern "C" nm_status nm_scalar_math_batch(uint64_t op, uint64_t n, const double* d_a, const double* d_b, double* d_out, void* stream) {
    nm_status st = ensure_device(-1);
    if (st != NM_OK) return st;
    if (op > 9 || op == 6) return fail(NM_ERR_INVALID_ARG, "unknown op");
    if (n == 0) return NM_OK;
    hipLaunchKernelGGL(scalar_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, n, d_a, d_b, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return NM_OK;
}

extern "C" nm_status nm_standard_normal_batch(uint64_t n, uint64_t count, const uint8_t* h_keys, double* d_out,
                                              uint64_t* h_words_consumed, void* stream) {
    nm_status st = ensure_device(-1);
    if (st != NM_OK) return st;
    if (!h_keys || !d_out) return fail(NM_ERR_INVALID_ARG, "null argument");
    if (n == 0 || count == 0) return NM_OK;
    std::vector<uint32_t> keys(8 * n);
    for (uint64_t i = 0; i < 8 * n; ++i)
        keys[i] = (uint32_t)h_keys[4 * i] | ((uint32_t)h_keys[4 * i + 1] << 8) | ((uint32_t)h_keys[4 * i + 2] << 16) | ((uint32_t)h_keys[4 * i + 3] << 24);
    std::vector<double> t(zig_tables, zig_tables + 2 * 257);
    uint32_t* d_keys = nullptr; double* d_zig = nullptr; uint64_t* d_words = nullptr;
    HIP_TRY(hipMalloc(&d_keys, keys.size() * 4));
    HIP_TRY(hipMalloc(&d_zig, t.size() * 8));
    HIP_TRY(hipMalloc(&d_words, n * 8));
    HIP_TRY(copy_on((hipStream_t)stream, d_keys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(copy_on((hipStream_t)stream, d_zig, t.data(), t.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(normal_batch_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, count, d_keys, d_zig, d_zig + 257, d_out, d_words);
    hipError_t er = hipGetLastError();
    if (er == hipSuccess) er = hipStreamSynchronize((hipStream_t)stream);
    if (er == hipSuccess && h_words_consumed) er = copy_on((hipStream_t)stream, h_words_consumed, d_words, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_keys); (void)hipFree(d_zig); (void)hipFree(d_words);
    if (er != hipSuccess) return fail(NM_ERR_HIP, "standard_normal_batch: %s", hipGetErrorString(er));
    return NM_OK;
}
