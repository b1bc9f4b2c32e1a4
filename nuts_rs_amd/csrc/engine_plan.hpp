// engine_plan.hpp — everything the host decides about an engine, in one place: which kernel family and tiling serves it, its grids and
// scratch layout (plan_engine), whether a transformation given from outside runs on the matrix cores (plan_transform), and which launches
// serve a draw call (plan_draw).  Host code, pure: no HIP call, no getenv, no global, no allocation.  What the device has to say — the
// compute-unit count and the kernels' occupancies — reaches plan_engine through DeviceFacts, which nuts_engine.hip backs with the
// kernels' query launches and tests/cpp/engine_plan_check.hip with constants.  What the kernels fix — layouts, depth limits, size rules —
// comes from nuts_contract.hpp.  DESIGN.md's table of kernel families ("selected when") describes what this file computes.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "nuts_contract.hpp"
#include "dev_math.hpp"       // dlog, u2d, d2u: the restated logarithm of ln_max_step and the jitter scale

namespace nm {
namespace plan {

constexpr uint64_t NM_LANE_EARLY_GROUP_DRAWS = 20;   // an engine that chose the one-chain-per-lane kernels by itself runs this many first warm-up draws 8 chains per wavefront
constexpr uint64_t CL_SLICE = 4096;                  // elements of a chain one block owns when the chain is wider than one block

// The instantiation family of the one-chain-per-block kernels.  The VALUES are ABI: a density module built with NM_MODULE_VARIANTS receives
// them as the `variant` argument of nm_module_launch_variant, next to a KernelKind (nuts_contract.hpp) whose ORDER is ABI for the same reason.
// Neither may be renumbered without a new NM_ABI_VERSION.
enum KernelFamily : int {
    FAMILY_PLAIN = 0,         // Density
    FAMILY_LOW_RANK = 1,      // LrWrap<Density>: the low-rank transformation (kern_lr_*.hip)
    FAMILY_KINETIC = 2,       // KinWrap<Density>: the non-Euclidean trajectory kinds of NUTS, MCLMC (kern_kin_*.hip)
    FAMILY_CLUSTER = 3,       // several blocks per chain, dim > 4096 (kern_cluster.hip)
    FAMILY_CLUSTER_KINETIC = 4
};

// choose (DPL, W) for a dim; requested_dpl / requested_w = 0 means automatic (fewest waves, then smallest tile)
inline bool pick_tiling(uint64_t dim, uint64_t requested_dpl, uint64_t requested_w, int* dpl_out, int* w_out) {
    static const int combos[8][2] = {{2, 1}, {4, 1}, {8, 1}, {16, 1}, {8, 2}, {16, 2}, {4, 4}, {16, 4}};   // {DPL, W}
    for (auto& c : combos) {
        if (requested_dpl && (uint64_t)c[0] != requested_dpl) continue;
        if (requested_w && (uint64_t)c[1] != requested_w) continue;
        if ((uint64_t)c[0] * 64 * c[1] >= dim) { *dpl_out = c[0]; *w_out = c[1]; return true; }
    }
    return false;
}

// Which kernel family serves small chains, by density class, dim bucket and chain count: the table measured by tools/crossover_sweep.py
// (profiles/r05m_crossovers.json, round 5; leapfrogs/s after the warm-up, every family that applies, 1024 .. 65536 chains) instead of round 4's
// constants, which were K4's alone.
//   regular densities (iid / diagonal normal, 8 schools, the full-precision normal up to 32 dims, user modules): several chains per wavefront as
//     soon as there are more chains than one-chain-per-wavefront slots (x 2 .. x 7 from 4096 chains on); one chain per lane from 32768 chains for
//     dim <= 4 (16384: 8 per wavefront 3.3e9 against 2.4e9), from 49152 for dim 5 .. 10 (32768: 4.2e9 against 3.4e9 at dim 10, a tie at dim 8;
//     65536: 5.8e9 against 4.2e9);
//   Neal's funnel (ragged trees: a wavefront waits for its slowest chain): one chain per wavefront wins up to 32768 chains at dim 10 and at every
//     count measured at dim 50; 8 chains per wavefront only for dim <= 16 from 49152 chains on (65536: 6.9e8 against 4.8e8); never one chain per lane.
struct SmallChainChoice { bool group, lane; };
inline SmallChainChoice small_chain_rule(uint64_t logp_kind, uint64_t dim, uint64_t n_chains, uint64_t wave_slots) {
    if (logp_kind == NM_LOGP_FUNNEL) return {dim <= 16 && n_chains >= 49152, false};
    return {n_chains > wave_slots, n_chains >= (dim <= 4 ? 32768u : 49152u)};
}

// What the device answers.  Every method returns false on failure, with `status` / `error` saying why; plan_engine then returns them.
struct DeviceFacts {
    nm_status status = NM_ERR_HIP;
    std::string error;
    virtual ~DeviceFacts() = default;
    virtual bool ready() = 0;                                  // asked once the configuration itself is accepted, before any other question
    virtual bool cu_count(int* cus) = 0;
    // resident blocks per compute unit of: the draw kernel of a family and tiling (K_QUERY); the several-chains-per-wavefront kernels
    // (K_GROUP_QUERY; family: plain or kinetic); the one-chain-per-lane kernels
    virtual bool wave_occupancy(KernelFamily family, int dpl, int wpc, int* occ) = 0;
    virtual bool group_occupancy(KernelFamily family, int dpl, int wpc, int* occ) = 0;
    virtual bool lane_occupancy(bool kinetic, int* occ) = 0;
};

// NM_LOGP_MODULE: the eight words of the module's nm_module_info and which optional entry points it exports
struct ModuleFacts {
    uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // sizeof(KParams), ABI version, doubles per lane, waves, lanes per chain of its group form, built for wide chains, lane form, variants
    bool has_launch_lane = false, has_launch_variant = false;
};

struct PlanInput {
    nm_settings s;                 // the caller's
    uint64_t logp_kind = 0, dim = 0, n_params = 0, n_chains = 0;
    nm_engine_config cfg;
    ModuleFacts module;
    DeviceFacts* dev = nullptr;
};

struct EnginePlan {
    nm_settings s;                 // normalised (MCLMC: the fixed step size and the Euclidean trajectory kind of its NUTS fields)
    nm_engine_config cfg;
    uint64_t logp_kind = 0, dim = 0, n_chains = 0;
    bool lr = false, kin = false, mclmc = false;
    // family and tiling
    KernelFamily family = FAMILY_PLAIN;
    int dpl = 0, wpc = 1;          // doubles per lane, waves per chain
    uint64_t dpad = 0;             // 64 x dpl x wpc
    uint64_t cl_k = 1;             // blocks per chain (dim > 4096: each with its own persistent vectors and copy of the scalars)
    uint64_t n_clusters = 0;
    bool sampling_build = false;   // the draw launches are of a family and tiling that has the sampling-phase build (nuts_kernels.hpp has_sampling_build)
    int module_group_lanes = 0;    // lanes per chain of a module's group form (0: it has none)
    // scratch layout
    uint64_t nsslot_tree = 0;      // the tree's scratch slots: what the lane kernel and the tile kernels use (no ring: ADVICE r03)
    uint64_t nsslot = 0;           // ... with the ring of batched merges and the sampling build's log of leaf weights: the stride between wavefronts
    uint64_t merge_counter_at = 0; // sampling_build: index in a wave's scratch of its count of exact-path merges
    uint64_t scratch_slots = 0;    // wavefronts' worth of scratch: the largest grid that uses it
    uint64_t lane_nslots = 0;      // the lane kernel's own scratch: slots, and pairs of doubles per chain
    int lane_np = 0;
    // grids (0: the family does not serve this engine)
    unsigned n_waves = 0;          // one chain per block: resident blocks
    unsigned group_grid = 0;       // several chains per wavefront (nuts_group.hpp)
    bool group_roomy = false;      // ... at most one wavefront per SIMD: the kernels compiled for that (K_GROUP_*_ROOMY)
    unsigned lane_grid = 0;        // one chain per lane (nuts_lane.hpp); takes precedence over the groups
    unsigned early_group_grid = 0; // with lane_grid, automatic choice only: the first NM_LANE_EARLY_GROUP_DRAWS warm-up draws run on the group kernels
    unsigned tile_grid = 0;        // the matrix-core kernels: 16-chain tiles on resident blocks
    bool tile_diag = false;        // DiagNutsSettings on the full-precision normal: P x on the matrix cores, per-chain mass matrices
    // low rank: eigenvector slots per chain, rows of a chain's window
    uint64_t lr_rmax = 0, lr_cap = 0;
    // derived scalars of KParams
    uint64_t early_end = 0, final_step_size_window = 0, mclmc_switch_draw = 0;
    double ln_max_step = 0.0, jitter_low = 0.0, jitter_scale = 0.0;
};

namespace detail {
inline std::string format(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
}  // namespace detail
#define NM_PLAN_REFUSE(st, ...) do { *status = (st); *why = detail::format(__VA_ARGS__); return p; } while (0)
#define NM_PLAN_ASK(call) do { if (!(call)) { *status = in.dev->status; *why = in.dev->error; return p; } } while (0)

// The whole choice for one engine.  *status != NM_OK: refused, *why says why, the returned plan is not to be used.
inline EnginePlan plan_engine(const PlanInput& in, nm_status* status, std::string* why) {
    EnginePlan p;
    *status = NM_OK;
    why->clear();
    nm_settings s = in.s;
    const nm_engine_config& cfg = in.cfg;
    const uint64_t kind = in.logp_kind, dim = in.dim, n_chains = in.n_chains;
    // (the tree's slot families and pend tables are laid out for maxdepth + extra_doublings levels: nuts_contract.hpp layout_depth)
    if (s.maxdepth > (uint64_t)MAX_MAXDEPTH || s.extra_doublings > (uint64_t)MAX_MAXDEPTH || s.maxdepth + s.extra_doublings > (uint64_t)MAX_MAXDEPTH)
        NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "maxdepth %llu + extra_doublings %llu > %d", (unsigned long long)s.maxdepth, (unsigned long long)s.extra_doublings, MAX_MAXDEPTH);
    if (s.step_size_method > NM_STEP_FIXED) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "step_size_method %llu is not one of NM_STEP_*", (unsigned long long)s.step_size_method);
    // GlobalStrategy::new asserts (adapt_strategy.rs:83-84)
    const double num_tune_f = (double)s.num_tune;
    const uint64_t step_size_window = (uint64_t)(s.step_size_window * num_tune_f);
    const uint64_t early_end = (uint64_t)(s.early_window * num_tune_f);
    if (!(early_end < s.num_tune)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "early_end < num_tune violated (reference asserts, adapt_strategy.rs:83)");
    if (!(s.mass_matrix_window_growth >= 1.0)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "mass_matrix_window_growth must be >= 1");
    if (s.has_jitter && !(1.0 - s.jitter < 1.0 + s.jitter)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "invalid jitter");
    if (s.adaptation > NM_ADAPT_LOW_RANK) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "adaptation %llu is not one of NM_ADAPT_*", (unsigned long long)s.adaptation);
    const bool lr = s.adaptation == NM_ADAPT_LOW_RANK;
    if (lr && !(s.lr_gamma > 0.0)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "lr_gamma must be > 0");
    if (s.trajectory_kind > NM_TRAJ_MICROCANONICAL) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "trajectory_kind %llu is not one of NM_TRAJ_*", (unsigned long long)s.trajectory_kind);
    if (s.sampler > NM_SAMPLER_MCLMC) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "sampler %llu is not one of NM_SAMPLER_*", (unsigned long long)s.sampler);
    const bool mclmc = s.sampler == NM_SAMPLER_MCLMC;
    if (mclmc) {
        if (s.mclmc_trajectory_kind > NM_MCLMC_EUCLIDEAN_EARLY_THEN_MICROCANONICAL) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "mclmc_trajectory_kind %llu is not one of NM_MCLMC_*", (unsigned long long)s.mclmc_trajectory_kind);
        if (!(s.mclmc_step_size > 0.0) || !(s.momentum_decoherence_length > 0.0)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "mclmc_step_size and momentum_decoherence_length must be > 0");
        if (dim < 2) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "ESH dynamics requires at least 2 dimensions (reference src/math/cpu_math.rs:514)");
        // DiagMclmcSettings::new_chain: adapt_options.step_size_settings.adapt_options.method = Fixed(self.step_size) (sampler.rs:421-423)
        s.step_size_method = NM_STEP_FIXED; s.fixed_step_size = s.mclmc_step_size;
        s.trajectory_kind = NM_TRAJ_EUCLIDEAN;      // (a NutsSettings field; MclmcChain's kind lives in the chain state)
    }
    const bool kin = mclmc || s.trajectory_kind != NM_TRAJ_EUCLIDEAN;
    if (s.trajectory_kind == NM_TRAJ_MICROCANONICAL && dim < 2) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "ESH dynamics requires at least 2 dimensions (reference src/math/cpu_math.rs:514)");
    if (cfg.lane_chains == 3) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "lane_chains = 3 (unsynchronised draws in the one-chain-per-lane kernels) was measured slower in every configuration and is removed (round 5); use 0 (automatic) or 2");

    // ---- tiling ----
    int dpl = 0, wv = 0;
    uint64_t cl_k = 1;
    constexpr uint64_t CL_MAX_K = CL_MAX_MEMBERS;
    // The matrix-core kernels (nuts_tile.hpp) exist for the 4-doubles-per-lane tiling only: an engine that may run them (full-precision
    // normal, 32 < dim <= 128, automatic tiling) takes that tiling for ALL its kernels — the same bits (elements 2 t, 2 t + 1 sit on
    // thread t either way; the second pair of a lane is padding, a +0.0 partial).  The 2-doubles instantiation of the tile kernels
    // was miscompiled by a rebuild in round 4 (garbage n_steps from draw 0; tools/probes/tile_dpl2_probe.py) and is not built any more.
    // (an explicit request for the several-chains-per-wavefront kernels, lane_groups == 2, keeps their 2-doubles tiling)
    // (only engines that can actually reach a matrix-core kernel — a FROZEN shared transformation, the per-chain diagonal
    // adaptation on >= 256 chains, or an explicit request — not every low-rank engine: a per-chain adapting run at dim <= 128 keeps its lanes busy)
    const bool may_tile = (lr ? s.freeze_transform != 0 : n_chains >= 256) || cfg.chain_tiles >= 2;
    const uint64_t auto_dpl = (kind == NM_LOGP_MVN_PREC && !cfg.dims_per_lane && !cfg.waves_per_chain && cfg.chain_tiles != 1 && cfg.lane_groups != 2 &&
                               may_tile && (dim > 32 || cfg.chain_tiles >= 2) && dim <= 128) ? 4 : cfg.dims_per_lane;
    if (dim > CL_SLICE) {     // wider than one block: ceil(dim / 4096) blocks per chain (kern_cluster.hip)
        cl_k = (dim + CL_SLICE - 1) / CL_SLICE;
        if (cl_k > CL_MAX_K) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "dim %llu > %llu", (unsigned long long)dim, (unsigned long long)(CL_SLICE * CL_MAX_K));
        if (kind != NM_LOGP_IID_NORMAL && kind != NM_LOGP_DIAG_NORMAL && kind != NM_LOGP_HOST_CALLBACK && kind != NM_LOGP_MODULE)
            NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "dim %llu > 4096: chains wider than one block exist for the element-wise densities (iid / diagonal normal), for density modules built for wide chains and for NM_LOGP_HOST_CALLBACK", (unsigned long long)dim);
        if (kind == NM_LOGP_MODULE && kin) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "density modules carry the Euclidean NUTS kernels only");
        if (lr) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "dim %llu > 4096: the diagonal adaptation only", (unsigned long long)dim);
        if ((cfg.dims_per_lane && cfg.dims_per_lane != 16) || (cfg.waves_per_chain && cfg.waves_per_chain != 4))
            NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "dim %llu > 4096 runs on the (16 doubles, 4 waves) tiling", (unsigned long long)dim);
        dpl = 16; wv = 4;
    } else if (!pick_tiling(dim, kind == NM_LOGP_EIGHT_SCHOOLS ? 2 : auto_dpl, kind == NM_LOGP_EIGHT_SCHOOLS ? 1 : cfg.waves_per_chain, &dpl, &wv))
        NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "no tiling for dim %llu with dims_per_lane %llu / waves_per_chain %llu (max dim 4096 = 16 doubles x 64 lanes x 4 waves)",
                       (unsigned long long)dim, (unsigned long long)cfg.dims_per_lane, (unsigned long long)cfg.waves_per_chain);
    NM_PLAN_ASK(in.dev->ready());

    p.s = s; p.cfg = cfg; p.logp_kind = kind; p.dim = dim; p.n_chains = n_chains;
    p.lr = lr; p.kin = kin; p.mclmc = mclmc;
    p.dpl = dpl; p.wpc = wv; p.cl_k = cl_k;
    p.family = cl_k > 1 ? (kin ? FAMILY_CLUSTER_KINETIC : FAMILY_CLUSTER) : lr ? FAMILY_LOW_RANK : (kin ? FAMILY_KINETIC : FAMILY_PLAIN);
    // (whether the launches are this family's at all — not the lane / group / matrix-core kernels — is decided in plan_draw)
    p.sampling_build = p.family == FAMILY_PLAIN && sampling_tiling(dpl, wv) && sampling_logp_kind(kind) &&
                       layout_depth(s) <= NM_MF_MAX_MD;      // (deeper layouts than its merge filter's error bound covers stay on the general kernel)
    const uint64_t dpad = 64ull * (uint64_t)dpl * (uint64_t)wv;
    p.dpad = dpad;
    // (tilings with batched merges keep the z of the last NM_RING leaves behind the tree's other scratch slots: the kernels' own predicate.
    // `plain` is "not several blocks per chain" here and !NM_TILE_MODE && !NM_CLUSTER_MODE in a kernel unit: tile mode needs no term on this
    // side: a tile engine takes P.nsslot as the stride between wavefronts like every other and never addresses the ring, so at <= 4 doubles per
    // lane its ring slots are allocated and unused)
    p.nsslot_tree = (uint64_t)num_sslots(layout_depth(s));
    // (the sampling build's log of leaf weights, 2^layout_depth doubles and one u64 counter, behind the tree's slots of every wave: dev_math.hpp mf_fold)
    const uint64_t nsslot_log = p.sampling_build ? ((1ull << layout_depth(s)) + 1 + dpad - 1) / dpad : 0;
    p.nsslot = p.nsslot_tree + (batched_merges(dpl, wv, cl_k == 1) ? (uint64_t)NM_RING : 0) + nsslot_log;
    p.merge_counter_at = p.nsslot_tree * dpad + (1ull << layout_depth(s));

    // ---- a density module's facts ----
    if (kind == NM_LOGP_MODULE) {
        const uint64_t* mi = in.module.info;
        p.module_group_lanes = (int)mi[4];
        if (lr && !((mi[7] & 1) && in.module.has_launch_variant)) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "NM_ADAPT_LOW_RANK with a density module built without the low-rank kernels: rebuild it with -DNM_MODULE_VARIANTS=1 (build_density_module(..., variants=(\"low_rank\",)))");
        if (kin && !lr && !((mi[7] & 2) && in.module.has_launch_variant)) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "the non-Euclidean trajectory kinds / NM_SAMPLER_MCLMC with a density module built without those kernels: rebuild it with -DNM_MODULE_VARIANTS=2 (build_density_module(..., variants=(\"kinetic\",)))");
        if ((mi[5] != 0) != (cl_k > 1)) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, cl_k > 1 ? "dim %llu > 4096 needs a density module built for wide chains (-DNM_CLUSTER_MODE=1, init_slice)" : "this density module was built for wide chains (dim > 4096), dim is %llu", (unsigned long long)dim);
        if (mi[0] != sizeof(KParams) || mi[1] != NM_ABI_VERSION) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "density module built against another engine (kernel parameters %llu bytes / ABI %llu, engine %zu / %d)", (unsigned long long)mi[0], (unsigned long long)mi[1], sizeof(KParams), NM_ABI_VERSION);
        if ((int)mi[2] != dpl || (int)mi[3] != wv) NM_PLAN_REFUSE(NM_ERR_INVALID_ARG, "density module was built for tiling (%llu doubles per lane, %llu waves) but dim %llu uses (%d, %d): rebuild it with nm_pick_tiling's answer", (unsigned long long)mi[2], (unsigned long long)mi[3], (unsigned long long)dim, dpl, wv);
    }

    // ---- grids ----
    int occ = 0, cus_ = 0;
    NM_PLAN_ASK(in.dev->wave_occupancy(p.family, dpl, wv, &occ));
    NM_PLAN_ASK(in.dev->cu_count(&cus_));
    const uint64_t cus = (uint64_t)(cus_ > 0 ? cus_ : 1);
    {   // one wave per resident slot of the chip (waves stride over the chains); tree scratch belongs to the wave
        uint64_t resident = (uint64_t)(occ > 0 ? occ : 1) * cus;
        const uint64_t wave_slots = resident;                       // chains the wave-per-chain kernel runs at once
        if (cfg.grid_blocks) resident = cfg.grid_blocks;            // tuning override: blocks in the grid
        p.n_waves = (unsigned)(n_chains < resident ? n_chains : resident);
        if (cl_k > 1) {     // whole clusters only, 8 x cl_k blocks at a time (block -> (cluster, member) map of the kernels); never
            const uint64_t unit = 8 * cl_k;                                  // more blocks than the chip holds at once (the members spin)
            uint64_t units = resident / unit;
            if (units == 0) NM_PLAN_REFUSE(NM_ERR_UNSUPPORTED, "dim %llu needs %llu co-resident blocks, the device holds %llu", (unsigned long long)dim, (unsigned long long)unit, (unsigned long long)resident);
            const uint64_t need = (n_chains + 7) / 8;
            if (units > need) units = need;
            p.n_waves = (unsigned)(units * unit);
            p.n_clusters = units * 8;
        }
        // small chains, more of them than the chip has wavefront slots: several chains per wave (nuts_group.hpp)
        const int gs = grp::group_size(dim);
        const bool group_density = (kind != NM_LOGP_MODULE && kind != NM_LOGP_HOST_CALLBACK) || (kind == NM_LOGP_MODULE && gs && p.module_group_lanes == gs);   // every built-in density has a group form
        // (the full-precision normal beyond 32 dims is faster on the matrix cores than two chains per wavefront: 3.7e8 against 3.0e8
        // leapfrogs/s at dim 64, tools/probes/mvn_small_dims.py)
        const bool mvn_tiles = !kin && kind == NM_LOGP_MVN_PREC && dim > 32 && cfg.chain_tiles != 1 && n_chains >= 256 && cfg.lane_groups != 2;
        // (the non-Euclidean trajectory kinds of NUTS and MCLMC's draw loop have group forms since round 4)
        if (cl_k == 1 && !lr && !mvn_tiles && cfg.lane_groups != 1 && group_density && gs && dim >= 1 && (gs == 8 || kind != NM_LOGP_EIGHT_SCHOOLS) && dpl == 2 && wv == 1 &&
            s.maxdepth + s.extra_doublings <= (uint64_t)grp::GMAXDEPTH && (small_chain_rule(kind, dim, n_chains, wave_slots).group || cfg.lane_groups == 2)) {   // measured: profiles/r05m_crossovers.json
            int gocc = 0;
            NM_PLAN_ASK(in.dev->group_occupancy(kin ? FAMILY_KINETIC : FAMILY_PLAIN, dpl, wv, &gocc));
            uint64_t gres = (uint64_t)(gocc > 0 ? gocc : 1) * cus;
            if (cfg.grid_blocks) gres = cfg.grid_blocks;
            const uint64_t need = (n_chains + (64 / gs) - 1) / (64 / gs);
            p.group_grid = (unsigned)(need < gres ? need : gres);
            // a grid that leaves every SIMD at most one wavefront (K4's shard: 8192 chains = 1024 wavefronts) runs the kernels whose register
            // allocation assumes just that (built-in densities, every sampler that has a group form; measured 1.47e9 -> 1.61e9 leapfrogs/s on K4's shard)
            p.group_roomy = kind != NM_LOGP_MODULE && (uint64_t)p.group_grid <= 4ull * cus;
        }
    }
    {   // very small chains, very many of them: one chain per LANE (nuts_lane.hpp); takes precedence over the lane groups
        const int np = lane::lane_pairs(dim);
        const bool dens_ok = kind == NM_LOGP_IID_NORMAL || kind == NM_LOGP_DIAG_NORMAL || kind == NM_LOGP_FUNNEL ||
                             (kind == NM_LOGP_EIGHT_SCHOOLS && dim == 10) ||
                             (kind == NM_LOGP_MODULE && in.module.has_launch_lane);      // a user density with a lane form
        // (the trajectory kinds of NUTS have lane forms for the built-in densities, in the synchronised kernel: round 4)
        const bool lane_kin_ok = !kin || (!mclmc && kind != NM_LOGP_MODULE);
        if (cl_k == 1 && !lr && lane_kin_ok && np && dens_ok && dim >= 1 && dpl == 2 && wv == 1 &&       // (the default tiling of these dims: its summation order is the lane kernel's)
            s.maxdepth + s.extra_doublings <= (uint64_t)lane::LMAXDEPTH && cfg.lane_chains != 1 &&      // (the pend table's levels: nuts_lane.hpp LaneShared)
            (cfg.lane_chains >= 2 || (cfg.lane_groups != 2 && np <= 5 && small_chain_rule(kind, dim, n_chains, 0).lane))) {   // (an explicit lane_groups == 2 wins over the automatic rule)
            // measured crossovers against the 8-lane kernels: small_chain_rule above (round 3: profiles/r03t_lane_group_crossover.txt);
            // the 8-pair kernel (dim 11 .. 16, 2 KB of scratch per lane) loses at every size measured and is only taken on request
            int locc = 0;
            NM_PLAN_ASK(in.dev->lane_occupancy(kin, &locc));
            uint64_t lres = (uint64_t)(locc > 0 ? locc : 1) * cus;
            if (cfg.grid_blocks) lres = cfg.grid_blocks;
            const uint64_t need = (n_chains + 63) / 64;
            p.lane_grid = (unsigned)(need < lres ? need : lres);
            // (automatic choice, built-in density, Euclidean NUTS: the group kernels keep their grid for the warm-up's first draws)
            p.early_group_grid = (cfg.lane_chains == 0 && !kin && kind != NM_LOGP_MODULE) ? p.group_grid : 0;
            p.group_grid = 0;
            p.lane_nslots = p.nsslot_tree;     // (the lane kernel never touches the ring)
            p.lane_np = np;
        }
    }
    {   // the matrix-core kernel's grid: 16-chain tiles on resident blocks (one 16-wave block fills a CU's wave slots)
        const uint64_t n_tiles = (n_chains + NM_TILE_CHAINS - 1) / NM_TILE_CHAINS;
        p.tile_grid = (unsigned)std::min<uint64_t>(n_tiles, cus * NM_TILE_OCC);
    }
    p.scratch_slots = p.n_waves > p.group_grid ? p.n_waves : p.group_grid;
    if (p.early_group_grid > p.scratch_slots) p.scratch_slots = p.early_group_grid;
    if (kind == NM_LOGP_MVN_PREC && cfg.chain_tiles != 1) p.scratch_slots = std::max<uint64_t>(p.scratch_slots, (uint64_t)p.tile_grid * NM_TILE_CHAINS);
    // DiagNutsSettings on the full-precision normal: the density's P is shared by all chains whatever their mass matrices are,
    // so P x can run on the matrix cores 16 chains at a time (nuts_tile_diag_kernel) — same bits as the one-chain GEMV.
    // chain_tiles: 0 = when there are enough chains to fill the blocks, 1 = never, 2 = whenever it applies
    p.tile_diag = !lr && !kin && cl_k == 1 && kind == NM_LOGP_MVN_PREC && cfg.chain_tiles != 1 && wv == 1 && dpl == 4 &&
                  dim <= 256 && p.group_grid == 0 && (cfg.chain_tiles == 2 || n_chains >= 256);      // (any dim: the packed P is zero-padded)
    if (lr) {
        // the estimator's rank is <= min(dim, 2 n_draws); a transformation given from outside may have any rank <= dim
        const uint64_t most = s.freeze_transform ? dim : std::min<uint64_t>(dim, 2 * (s.num_tune + 1));
        p.lr_rmax = cfg.lowrank_max_rank ? std::min<uint64_t>(cfg.lowrank_max_rank, dim) : most;
        if (p.lr_rmax == 0) p.lr_rmax = 1;
        p.lr_cap = s.num_tune + 2;
    }

    // ---- derived scalars of KParams ----
    p.early_end = early_end;
    {   // MclmcChain's switch_draw = (trajectory_switch_fraction * num_tune) as u64 (sampler.rs:441; `as` saturates, NaN -> 0)
        const double q = s.trajectory_switch_fraction * num_tune_f;
        p.mclmc_switch_draw = q >= 18446744073709551616.0 ? ~0ull : (q > 0.0 ? (uint64_t)q : 0ull);
    }
    p.final_step_size_window = s.num_tune >= step_size_window ? s.num_tune - step_size_window : 0;   // saturating_sub
    p.ln_max_step = dlog(s.da_max_step_size);
    if (s.has_jitter) {   // Uniform::new(1 - j, 1 + j)
        const double low = 1.0 - s.jitter, high = 1.0 + s.jitter, max_rand = 1.0 - 2.220446049250313e-16;
        double scale = high - low;
        while (scale * max_rand + low >= high) scale = u2d(d2u(scale) - 1);
        p.jitter_low = low; p.jitter_scale = scale;
    }
    return p;
}
#undef NM_PLAN_REFUSE
#undef NM_PLAN_ASK

// A transformation given from outside (nm_engine_set_transform): one for all chains, frozen, on the full-precision normal, can run 16
// chains per block with U', U and P on the matrix cores (nuts_tile.hpp) — on the lockstep form of that kernel or on the one-wavefront-per-
// chain tile kernel.  The choice is made once per call: the two kernels sum over dim in different orders.  Every call decides afresh
// (a later call that does not qualify must not leave the lockstep order reported).
struct TransformPlan {
    bool tile = false;             // the matrix-core kernels serve the draws (their matrices are to be packed and uploaded)
    bool lock = false;             // ... the lockstep form (reductions in ITS order: nm_engine_reduce_order)
    nm_status status = NM_OK;      // chain_tiles = 3 that cannot be honoured: `tile` / `lock` stand as computed, the call returns this
    const char* why = "";
};
// update_ok: the transformation was accepted (finite input)
inline TransformPlan plan_transform(const EnginePlan& p, bool per_chain, uint64_t n_eig, uint64_t dim, bool update_ok) {
    TransformPlan t;
    const nm_settings& s = p.s;
    if (!per_chain && s.freeze_transform && s.trajectory_kind == NM_TRAJ_EUCLIDEAN && s.sampler == NM_SAMPLER_NUTS && p.logp_kind == NM_LOGP_MVN_PREC && p.cfg.chain_tiles != 1 && p.wpc == 1 &&
        p.dpl == 4 && dim <= 256 && n_eig >= 8 && n_eig <= 256 && dim % 8 == 0 && n_eig % 8 == 0 && update_ok) {
        t.tile = true;
        // chain_tiles: 0 = the lockstep kernel where it applies, else the one-wavefront-per-chain tile kernel; 2 = always the latter;
        // 3 = the lockstep kernel or an error
        const bool lock_ok = s.maxdepth >= 1 && s.maxdepth + s.extra_doublings <= (uint64_t)lock::LOCK_MAXDEPTH;
        // (an engine whose settings ask for the divergence / mass-matrix vectors — outputs the lockstep kernel does not write —
        // takes the tile kernel when the choice is automatic; an explicit chain_tiles = 3 keeps the lockstep kernel and its error)
        const bool wants_vectors = s.store_divergences || s.store_mass_matrix;
        t.lock = lock_ok && ((p.cfg.chain_tiles == 0 && !wants_vectors) || p.cfg.chain_tiles == 3);
        if (p.cfg.chain_tiles == 3 && !t.lock) { t.status = NM_ERR_UNSUPPORTED; t.why = "chain_tiles = 3: the lockstep kernel needs maxdepth + extra_doublings <= 11"; }
    } else if (p.cfg.chain_tiles == 3) {
        t.status = NM_ERR_UNSUPPORTED;
        t.why = "chain_tiles = 3: the lockstep kernel serves one shared, frozen transformation on the full-precision normal (dim, rank multiples of 8, <= 256)";
    }
    return t;
}
// why a draw call that asks the lockstep kernel for the divergence / mass-matrix vectors is refused
inline const char* lockstep_outputs_error(const EnginePlan& p) {
    return p.cfg.chain_tiles == 0 ?
        "this engine chose the lockstep matrix-core kernel (settings without store_divergences / store_mass_matrix), which writes positions, "
        "statistics, gradient and the transformed point only; set store_divergences / store_mass_matrix in the settings (the engine then "
        "takes the tile kernel from the start: the two sum over dim in different orders) or chain_tiles = 2" :
        "the lockstep matrix-core kernel writes positions, statistics, gradient and the transformed point only; "
        "create the engine with chain_tiles = 2 for the divergence / mass-matrix vectors";
}

// ---- the launches of one draw call ----
enum class Launch {
    Wave,            // one chain per block, the general draw kernel of the engine's family (K_DRAW)
    WaveSampling,    // ... its sampling-phase build (K_DRAW_SAMPLING)
    Group,           // several chains per wavefront (K_GROUP_TUNE / K_GROUP_DRAW, `roomy`: their _ROOMY builds)
    Lane,            // one chain per lane
    TileDiag,        // matrix cores, per-chain diagonal mass matrices
    TilePrec,        // matrix cores, the shared low-rank transformation
    Lockstep         // ... its lockstep form
};
struct LaunchStep {
    Launch what;
    unsigned grid;
    uint64_t n_draws;
    bool tune;       // Group / Lane: the launch starts inside the warm-up and takes the kernel with the adaptation compiled in
    bool roomy;      // Group
};
struct DrawState {
    uint64_t draws_launched = 0;   // draw index of the healthy chain that is furthest behind
    // The sampling-phase build serves the draws from this index on: num_tune + 1 (draw num_tune runs the last `adapt` transition of the
    // warm-up and may re-whiten after the final mass-matrix update; after it every chain has tuning = 0, mm_id == transform_id and a
    // frozen step-size state), and after a set_position one draw past the current one (the general kernel's draw re-whitens, replaces
    // the step size of the search by the adapted one and reports the new mass matrix; from then on the state is frozen again).
    uint64_t sampling_from = 0;
    TransformPlan transform;
};
struct DrawPlan { int n = 0; LaunchStep step[2]; };

inline uint64_t sampling_from_after_set_position(const EnginePlan& p, uint64_t draws_launched) { return std::max<uint64_t>(p.s.num_tune, draws_launched) + 1; }

// At most two steps, in order, whose draws sum to n_draws (n_draws > 0); the second step's output rows follow the first's.
inline DrawPlan plan_draw(const EnginePlan& p, const DrawState& d, uint64_t n_draws) {
    DrawPlan out;
    auto add = [&out](Launch what, unsigned grid, uint64_t n, bool tune = false, bool roomy = false) { if (n) out.step[out.n++] = {what, grid, n, tune, roomy}; };
    const uint64_t at = d.draws_launched, num_tune = p.s.num_tune;
    if (p.lr) {        // (no small-chain or sampling form carries the low-rank transformation)
        if (d.transform.tile) add(d.transform.lock ? Launch::Lockstep : Launch::TilePrec, p.tile_grid, n_draws);
        else add(Launch::Wave, p.n_waves, n_draws);
    } else if (p.lane_grid) {
        // The first draws of a warm-up (step sizes straight from the initial search: trees to depth 10 somewhere in every 64-chain wavefront)
        // on the 8-lanes-per-chain kernels, the rest of the call one chain per lane: the same draws either way (both kernels are the
        // oracle's bits), measured on K4's 65536 chains launch by launch (profiles/r04z_k4_warmup_chunks.jsonl).
        uint64_t n1 = 0;
        if (p.early_group_grid && at < NM_LANE_EARLY_GROUP_DRAWS && at < num_tune) n1 = std::min<uint64_t>(n_draws, NM_LANE_EARLY_GROUP_DRAWS - at);
        add(Launch::Group, p.early_group_grid, n1, /*tune=*/true);
        add(Launch::Lane, p.lane_grid, n_draws - n1, at + n1 < num_tune);
    } else if (p.group_grid) {
        add(Launch::Group, p.group_grid, n_draws, at < num_tune, p.group_roomy);
    } else if (p.tile_diag) {
        add(Launch::TileDiag, p.tile_grid, n_draws);
    } else {
        // the draws below index sampling_from on the general kernel, the rest on the sampling-phase build (same stream, one grid, rows as of one launch)
        const uint64_t n_general = !p.sampling_build ? n_draws : at >= d.sampling_from ? 0 : std::min<uint64_t>(n_draws, d.sampling_from - at);
        add(Launch::Wave, p.n_waves, n_general);
        add(Launch::WaveSampling, p.n_waves, n_draws - n_general);
    }
    return out;
}

}  // namespace plan
}  // namespace nm
