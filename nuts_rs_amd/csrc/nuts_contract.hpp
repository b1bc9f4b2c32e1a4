// nuts_contract.hpp — what host code and at least one kernel unit must agree on, stated once: the memory layouts, the per-chain scalars,
// the kernel parameters, the kernel kinds, the depth limits and size rules of every kernel family, and the launch entry points.
// Declarations and small host/device functions only: no device intrinsic, no register tile, nothing that depends on a unit's mode
// (NM_TILE_MODE, NM_CLUSTER_MODE, NM_TU_PART, NM_DETMATH_INLINE), so every unit in every mode includes it and a plain host compiler
// accepts it (tests/cpp/contract_check.cpp).  The kernel headers include it and say what they do with these facts.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <type_traits>
#include "../../include/nuts_amd.h"
// chains per block of the matrix-core kernels (nuts_tile.hpp) and their blocks per compute unit; tuning builds pass both to all units
#ifndef NM_TILE_CHAINS
#define NM_TILE_CHAINS 16    // chains = wavefronts per block: 16 (all 16 columns of the f64 MFMA carry a chain) or 8 (half of them; tuning builds)
#endif
#ifndef NM_TILE_OCC
#define NM_TILE_OCC 1        // blocks per compute unit the register allocation leaves room for
#endif
namespace nm {
constexpr int MAX_MAXDEPTH = 20;
constexpr int CL_MAX_MEMBERS = 32;          // blocks per chain at most (dim <= 32 x 4096): the members of a chain share an XCD, which has 32 CUs
constexpr int NM_MF_MAX_MD = 12;            // deepest layout (maxdepth + extra_doublings) the merge filter's bound (dev_math.hpp NM_MF_EPS_MAX) is derived for: 2 * 12 + 2 = 26 merges in a chain
// ---------------------------------------------------------------------------------------------
// HBM layout.
//   pvec[chain][PSlot][DP]  : what a chain owns between draws
//   svec[wave][scratch][DP] : tree scratch of a resident wave
// ---------------------------------------------------------------------------------------------
enum PSlot : int {
    P_X = 0, P_GX, P_Z, P_GZ,          // current point (TransformedPoint, transformed_hamiltonian.rs:56-77)
    P_SIG, P_ISIG, P_MU,               // DiagMassMatrix stds / inv_stds / mean (transform/diagonal.rs:9-17)
    E_DM, E_DV, E_GM, E_GV,            // foreground RunningVariance of draws / grads (adapt/diagonal.rs:108-115)
    B_DM, B_DV, B_GM, B_GV,            // background
    P_V,                               // MclmcChain: the momentum survives from draw to draw (src/mclmc.rs:551)
    NUM_PSLOT
};
// main-tree edges: `left` and `right` are edge ids 0/1 (both start as the initial point's id 0; a successful doubling
// writes the new edge to the id this side owns alone, or to id 1 while both sides still share id 0).  Only the g_z of
// an edge lives here (EDGEn_G); its (z, v) stay in LDS (BlockShared::edge_z / edge_v).
enum SSlot : int { EDGE0_Z = 0, EDGE0_V, EDGE0_G, EDGE1_Z, EDGE1_V, EDGE1_G, EDGE2_Z, EDGE2_V, EDGE2_G, STAGE_V, S_DYN };
__host__ __device__ inline int slot_edge(int id) { return EDGE0_Z + 3 * id; }
// dynamic scratch: F[k] (z,v), L[k] (z,v) for k in 0..=maxdepth, then the candidate pool C[p] (z), p in 0..maxdepth+2
__host__ __device__ inline int slot_F(int k) { return S_DYN + 2 * k; }
__host__ __device__ inline int slot_L(int maxdepth, int k) { return S_DYN + 2 * (maxdepth + 1) + 2 * k; }
__host__ __device__ inline int slot_C(int maxdepth, int p) { return S_DYN + 4 * (maxdepth + 1) + p; }
__host__ __device__ inline int num_sslots(int maxdepth) { return S_DYN + 4 * (maxdepth + 1) + (maxdepth + 3); }
// Batched merges (DPL <= 4, one wave per chain; see resolve_chunk): the z of the last NM_RING leaves, one slot per leaf (leaf n of
// a doubling lives in slot n mod NM_RING), behind the slots above.  The host adds NM_RING to nsslot for these tilings.
constexpr int NM_RING = 64;
__host__ __device__ inline int slot_R(int maxdepth, int i) { return num_sslots(maxdepth) + i; }
// The depth every slot family (F, L, candidate pool, pend tables) is laid out for.  A tree that turned at depth d <= maxdepth is extended by
// `extra_doublings` further doublings (src/nuts.rs:350-371), so sub-trees of level up to maxdepth + extra_doublings - 1 are built; with the
// layout of `maxdepth` alone slot_L(MD, MD + 1) is slot_C(MD, 0) and the candidate pool overflows.
// (Computed once by the host into KParams::layout_md: reading both settings fields in ctx_begin changed the register allocation of the
// 16-wavefront matrix-core kernel enough to break it — the last doubling of trees deeper than 6 stopped after one leaf)
__host__ __device__ inline int layout_depth(const nm_settings& s) { return (int)(s.maxdepth + s.extra_doublings); }
// Batched merges (resolve_chunk): the one-wavefront tilings up to this width evaluate a doubling's merges together and keep a ring of the
// last NM_RING leaves behind the tree's other scratch slots.  ONE predicate for the kernels and for the host's scratch layout.
constexpr int NM_BATCH_MAX_DPL = 4;
__host__ __device__ constexpr bool batched_merges(int dpl, int w, bool plain) { return plain && w == 1 && dpl <= NM_BATCH_MAX_DPL; }
// Per-chain scalars (everything of NutsChain / GlobalStrategy / stepsize::Strategy / DualAverage that is not a vector)
struct ChainScalars {
    uint32_t key[8];
    uint64_t rng_pos;
    // current point
    double logp, logdet;
    int64_t transform_id;
    // mass matrix
    double mm_logdet;
    int64_t mm_id;
    // hamiltonian
    double step_size;
    // GlobalStrategy (adapt_strategy.rs:24-39)
    uint64_t draw_count, last_update, current_window_size, tuning, has_initial_mass_matrix;
    // RunningVariance counts (draw and grad estimators always have equal counts)
    uint64_t cnt_fg, cnt_bg;
    // DualAverage (dual_avg.rs:34-41)
    double log_step, log_step_adapted, hbar, mu;
    uint64_t da_count;
    // Adam (stepsize/adam.rs:42-53); its log_step shares `log_step` above
    double adam_m, adam_v;
    uint64_t adam_t;
    // stepsize::Strategy last_* (stepsize/adapt.rs:58-64)
    double last_mean_tree_accept, last_sym_mean_tree_accept, last_max_energy_error;
    uint64_t last_n_steps;
    uint64_t status;       // NM_CHAIN_*
    uint64_t total_steps;  // leapfrogs since creation (metric)
    uint64_t px_stale;     // 1: P_X / P_GX do not hold the current point (they equal what P_Z recomputes to)
    int64_t stats_last_id; // mass-matrix id at the previous statistics extraction (chain.rs:195-200), starts at -1
    // ---- low-rank transformation and its adaptation (NM_ADAPT_LOW_RANK; LrWrap kernels only)
    uint64_t lr_has_inner;        // LowRankMassMatrix.inner.is_some() (low_rank.rs:112)
    uint64_t lr_rank;             // InnerMatrix.num_eigenvalues
    // LowRankMassMatrixStrategy (adapt/low_rank.rs:14-21): the deque is rows [lr_start, lr_start + lr_len) of the chain's
    // window buffer; lr_split = background_split
    uint64_t lr_start, lr_len, lr_split;
    // hand-off with the host's estimator: 1 = GlobalStrategy::adapt paused at `mass_matrix_adapt.adapt(..)`, waiting;
    // 2 = the host answered (lr_upd_*); 3 = a transformation from nm_engine_set_transform waits to be committed
    uint64_t lr_pending;
    uint64_t lr_upd_ok, lr_upd_rank;   // the answer: a finite update was uploaded (P_SIG / P_ISIG / P_MU, lrvec, lrval), its rank
    double lr_upd_logdet;              // its -1/2 sum ln lambda (InnerMatrix::new, low_rank.rs:57)
    uint64_t lr_is_late;               // is_late of the paused adapt call
    uint64_t lr_row;                   // output row of the paused draw
    // KinWrap kernels: the Hamiltonian's current KineticEnergyKind (NutsSettings::trajectory_kind; MclmcChain switches it)
    uint64_t kin;
};
enum { LR_IDLE = 0, LR_WAIT_HOST = 1, LR_ANSWERED = 2, LR_SET_TRANSFORM = 3 };
struct KParams {
    nm_settings s;
    uint64_t n_chains, dim, dpad, chain_id_offset, nsslot;
    double* pvec;
    double* svec;
    ChainScalars* sc;
    const double* zig_x;
    const double* zig_f;
    const double* logp_params;
    // derived schedule constants (GlobalStrategy::new, adapt_strategy.rs:77-98)
    uint64_t early_end, final_step_size_window;
    uint64_t mclmc_switch_draw;        // MclmcChain::switch_draw (sampler.rs:441)
    // chains wider than one block (NM_CLUSTER_MODE kernels): cl_k members of cl_slice elements each per chain, their mailboxes
    uint64_t cl_k, cl_slice;
    uint64_t cl_general;               // 1: always the general (release / acquire) exchange, never the same-XCD one (NM_CLUSTER_GENERAL=1: tests)
    unsigned long long* cl_box;        // [clusters][2][cl_k][RED_MAX_VALUES]
    unsigned long long* cl_cnt;        // [clusters], zeroed before every launch
    double ln_max_step;                // ln(da_max_step_size), dual_avg.rs:59
    double jitter_low, jitter_scale;   // Uniform::new(1-j, 1+j) (stepsize/adapt.rs:259-261)
    // outputs of the draw kernel
    double* out_positions;       // [n_draws][n_chains][dim] or null
    nm_draw_stats* out_stats;    // [n_draws][n_chains] or null
    // vector-valued statistics (nm_draw_outputs), [n_draws][n_chains][dim] or null
    double *out_gradient, *out_tpos, *out_tgrad, *out_mm_inv, *out_mm_mu;
    double *out_div_start, *out_div_start_grad, *out_div_end;
    uint64_t n_draws;
    unsigned long long* prof;    // NM_PROF builds: cycle counters of block 0 (tools/prof_phases.py)
    const double* x0;            // init kernel: [n_chains][dim]
    // low-rank transformation (LrWrap kernels): per chain [1 + lr_rmax][dpad] (row 0 = mu_lr, row 1 + k = eigenvector k,
    // tile layout like every chain vector), [2][lr_rmax] (lambda^1/2, lambda^-1/2), and the window [lr_cap][2][dim]
    double* lrvec;
    double* lrval;
    double* lrwin;
    uint64_t lr_rmax, lr_cap;
    uint64_t draw_end, row_base;  // LrWrap draw kernel: chains draw until draw_count == draw_end; output row = draw_count - row_base
    double* out_mm_eigvals;
    const uint8_t* init_mask;     // init kernel: chains with mask 0 are left untouched (null = all)
    // NM_LOGP_HOST_CALLBACK: one mailbox per chain in pinned host memory (CbMail header, then x[dim], grad[dim])
    unsigned char* cb_mail;
    uint64_t cb_stride;           // bytes per mailbox
    uint64_t layout_md;           // layout_depth(s) = maxdepth + extra_doublings: the depth the tree's slot families are laid out for
};
struct CbMail { uint64_t req, resp; int64_t status; double logp; };      // (the protocol: nuts_kernels.hpp HostCb)
enum KernelKind { K_INIT, K_DRAW, K_QUERY,      // K_QUERY: resident blocks per CU of the draw kernel
                  K_GROUP_DRAW, K_GROUP_TUNE, K_GROUP_QUERY,    // the small-chain kernels of nuts_group.hpp (dim <= 64): sampling / warm-up
                  K_GROUP_DRAW_ROOMY, K_GROUP_TUNE_ROOMY,       // ... compiled for one wavefront per SIMD (grids of at most 4 x CUs blocks; built-in densities)
                  K_DRAW_SAMPLING };    // the draw kernel's sampling-phase build (nuts_kernels.hpp has_sampling_build): launches whose draws all have an index > num_tune.
                                        // (Last, so that the kinds a density module was built with keep their values; a module is never asked for this one.)
inline bool is_group_kind(KernelKind kind) { return kind == K_GROUP_DRAW || kind == K_GROUP_TUNE || kind == K_GROUP_QUERY || kind == K_GROUP_DRAW_ROOMY || kind == K_GROUP_TUNE_ROOMY; }
// The sampling-phase build of the one-chain-per-block draw kernel (K_DRAW_SAMPLING) exists for these tilings of these densities: the kernels
// ask by type (nuts_kernels.hpp has_sampling_build: plain_unit && tiling && type), the host by kind (engine_plan.hpp: its family and
// NM_MF_MAX_MD terms && tiling && kind).  The two lists name the same densities; a launch of a build that is missing fails.
struct IidNormal; struct DiagNormal; struct Funnel; struct MvnPrec;
constexpr bool sampling_tiling(int dpl, int w) { return w == 1 && (dpl == 8 || dpl == 16); }
constexpr bool sampling_logp_kind(uint64_t kind) { return kind == NM_LOGP_IID_NORMAL || kind == NM_LOGP_DIAG_NORMAL || kind == NM_LOGP_FUNNEL || kind == NM_LOGP_MVN_PREC; }
template <class Dens> constexpr bool sampling_density() {
    return std::is_same<Dens, IidNormal>::value || std::is_same<Dens, DiagNormal>::value || std::is_same<Dens, Funnel>::value ||
           std::is_same<Dens, MvnPrec>::value;          // (the 8 schools run on the 2-doubles tiling alone)
}
namespace grp {
constexpr int GMAXDEPTH = 10;
// lanes per chain for a dim (0: no group form)
__host__ __device__ inline int group_size(uint64_t dim) { return dim <= 16 ? 8 : dim <= 32 ? 16 : dim <= 64 ? 32 : 0; }
}  // namespace grp
namespace lane {
constexpr int LMAXDEPTH = 10;
// (round 5: the 8-pair kernel for dim 11 .. 16 — 2 KB of scratch per lane, slower than the 8-lane kernels at every size measured — is removed)
__host__ __device__ inline int lane_pairs(uint64_t dim) { return dim <= 4 ? 2 : dim <= 8 ? 4 : dim <= 10 ? 5 : 0; }
struct LaneParams {
    double* lws;          // [grid][NUM_PSLOT][2 NP][64]  the chains' persistent vectors while the kernel runs
    double* lsv;          // [grid][nslots][2 NP][64]     tree scratch
    uint64_t nslots;
};
}  // namespace lane
namespace lock { constexpr int LOCK_MAXDEPTH = 11; } // maxdepth + extra_doublings the kernel is laid out for (sums, pend table); the engine checks
namespace tile {
// The shared matrices in MFMA operand order.  For a product out[R x 16] = M[R x K] B[K x 16], stripe s (rows 16 s ..),
// k-pair q (inner indices 8 q .. 8 q + 7): packed[(s * kpairs + q) * 64 + lane] = { M[16 s + (lane & 15)][8 q + (lane >> 4)],
// M[16 s + (lane & 15)][8 q + 4 + (lane >> 4)] } — two A operands per 16-byte load, 1 KiB per wave instruction.
struct TileMats {
    const double* ut;        // M = U'  (rank x dim):  M[k][d] = vecs[k][d]
    const double* u;         // M = U   (dim x rank):  M[d][k] = vecs[k][d]
    const double* p;         // M[d][j] = P[j][d]      (the one-chain density's column order)
    int dim, rank;
    int dim_kp, rank_kp;     // k-pairs of inner length dim / rank (padded with zeros)
    int dim_st, rank_st;     // 16-row stripes of dim / rank outputs
};
}  // namespace tile
// ---- the launch entry points, each declared once.  A density's, in kern_<density>.hip: NM_DEFINE_LAUNCH(launch_x, Density) (nuts_launch.hpp)
// grid = number of blocks (one block of 64*W threads = one resident chain); for K_QUERY *occ receives
// hipOccupancyMaxActiveBlocksPerMultiprocessor of the draw kernel
#define NM_LAUNCH_ARGS int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ
// one definition per density, in kern_<density>.hip
hipError_t launch_iid_normal(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_diag_normal(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_funnel(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_eight_schools(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_mvn_prec(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// the same kernels with the low-rank transformation compiled in (LrWrap<Density>), in kern_lr_<density>.hip
hipError_t launch_iid_normal_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_diag_normal_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_funnel_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_eight_schools_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_mvn_prec_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// the same kernels with the non-Euclidean KineticEnergyKinds compiled in (KinWrap<Density>), in kern_kin_<density>.hip
hipError_t launch_iid_normal_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_diag_normal_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_funnel_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_eight_schools_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_mvn_prec_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_host_cb_kin(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// chains wider than one block (kern_cluster.hip): dim > 4096, element-wise densities
hipError_t launch_cluster(uint64_t logp_kind, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// ... with the non-Euclidean trajectory kinds / MCLMC (kern_cluster_kin.hip)
hipError_t launch_cluster_kin(uint64_t logp_kind, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// NM_LOGP_HOST_CALLBACK (kern_host_cb.hip)
hipError_t launch_host_cb(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_host_cb_lr(int dpl, int w, KernelKind kind, const KParams& P, unsigned grid, hipStream_t stream, int* occ);
// the matrix-core kernel for shared matrices lives in its own (tile-mode) translation unit: kern_tile_mvn_prec.hip
hipError_t launch_tile_mvn_prec(int dpl, int query, const KParams& P, const tile::TileMats& M, unsigned grid, hipStream_t stream, int* occ);
hipError_t launch_tile_mvn_diag(int dpl, const KParams& P, const tile::TileMats& M, unsigned grid, hipStream_t stream);
// the lockstep matrix-core kernel (nuts_lockstep.hpp, kern_lockstep.hip): 16 chains per block advance together, draws not synchronised
hipError_t launch_lockstep(int query, const KParams& P, const tile::TileMats& M, unsigned grid, hipStream_t stream, int* occ);
// the one-chain-per-lane kernels (kern_lane.hip)
hipError_t launch_lane(uint64_t logp_kind, int query, bool tune, const KParams& P, const lane::LaneParams& LP, unsigned grid, hipStream_t stream, int* occ);
// ... with the non-Euclidean trajectory kinds of NUTS compiled in (kern_lane_kin.hip; the synchronised form only)
hipError_t launch_lane_kin(uint64_t logp_kind, int query, bool tune, const KParams& P, const lane::LaneParams& LP, unsigned grid, hipStream_t stream, int* occ);
// kern_expand.hip: the built-in densities.  *has_kernel = 0: the expansion is the identity (edim == dim)
uint64_t builtin_expanded_dim(uint64_t logp_kind, uint64_t dim, const double* h_params, uint64_t n_params, int* has_kernel);
hipError_t launch_expand(uint64_t logp_kind, const double* d_params, uint64_t dim, uint64_t edim, uint64_t n_rows, const double* d_positions,
                         double* d_expanded, unsigned grid_cap, hipStream_t stream);
// lowrank_device.hip: the estimator as a kernel (one block per paused chain)
namespace lrb {
bool block_estimator_takes(uint64_t dim, uint64_t n_max);
size_t block_estimator_scratch_doubles(uint64_t dim, uint64_t n_max);
hipError_t launch_estimate(unsigned grid, hipStream_t stream, const uint64_t* d_jobs, uint64_t n_jobs, uint64_t dim, const double* d_lrwin, uint64_t lr_cap,
                           double gamma, double eigval_cutoff, double* d_scratch, uint64_t scratch_stride, double* d_rows, uint64_t rows, uint64_t dp,
                           double* d_vals2, uint64_t rmax, uint64_t* d_meta, unsigned long long* d_too_wide, void* d_sc, double* d_vals_plain);
}  // namespace lrb
}  // namespace nm
