// vector_plan_check.hip — HOST program (compiled with hipcc, runs on the CPU): csrc/engine_plan.hpp's answer for the cases of
// tests/test_gpu_vector_outputs.py.  One case per line on standard input:
//     id logp_kind dim n_chains dims_per_lane waves_per_chain lane_groups lane_chains chain_tiles adaptation freeze_transform trajectory_kind
//     sampler num_tune maxdepth store_divergences store_mass_matrix transform(0 none | 1 shared | 2 per chain) n_eig cut draws
// One line out per case: id status family doubles-per-lane waves blocks-per-chain, then the launches plan_draw names for the case's two
// calls (draws [0, cut) and [cut, draws)) as a sorted list of wave / sampling / group / lane / tile_diag / tile / lockstep.
// The device is engine_plan_check.hip's constant: 256 compute units, 8 resident blocks per unit of the wave and group kernels, 2 of the
// lane kernels.  tests/test_vector_output_matrix.py compares the lines with what the GPU cases assert.
#include "../../nuts_rs_amd/csrc/engine_plan.hpp"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
using namespace nm;
using namespace nm::plan;

struct Facts final : DeviceFacts {
    bool ready() override { return true; }
    bool cu_count(int* cus) override { *cus = 256; return true; }
    bool wave_occupancy(KernelFamily, int, int, int* occ) override { *occ = 8; return true; }
    bool group_occupancy(KernelFamily, int, int, int* occ) override { *occ = 8; return true; }
    bool lane_occupancy(bool, int* occ) override { *occ = 2; return true; }
};

static nm_settings diag_settings() {      // nm_settings_default's values of the fields the plan reads
    nm_settings s;
    memset(&s, 0, sizeof s);
    s.num_tune = 400; s.num_draws = 1000; s.maxdepth = 10; s.early_window = 0.3; s.step_size_window = 0.15; s.mass_matrix_window_growth = 1.5;
    s.has_jitter = 1; s.jitter = 0.1; s.da_max_step_size = 3.14159265358979323846; s.step_size_method = NM_STEP_DUAL_AVERAGE;
    s.adaptation = NM_ADAPT_DIAG; s.lr_gamma = 1e-5; s.lr_eigval_cutoff = 2.0; s.trajectory_kind = NM_TRAJ_EUCLIDEAN; s.sampler = NM_SAMPLER_NUTS;
    s.mclmc_step_size = 0.5; s.momentum_decoherence_length = 3.0; s.mclmc_trajectory_kind = NM_MCLMC_EUCLIDEAN_EARLY_THEN_MICROCANONICAL; s.trajectory_switch_fraction = 0.3;
    return s;
}

int main() {
    char id[256];
    unsigned long long v[20];
    for (;;) {
        if (scanf("%255s", id) != 1) break;
        for (auto& x : v) if (scanf("%llu", &x) != 1) { fprintf(stderr, "short line for %s\n", id); return 2; }
        Facts facts;
        PlanInput in;
        in.s = diag_settings();
        memset(&in.cfg, 0, sizeof in.cfg);
        in.cfg.device = -1;
        in.logp_kind = v[0]; in.dim = v[1]; in.n_chains = v[2];
        in.cfg.dims_per_lane = v[3]; in.cfg.waves_per_chain = v[4]; in.cfg.lane_groups = v[5]; in.cfg.lane_chains = v[6]; in.cfg.chain_tiles = v[7];
        in.s.adaptation = v[8]; in.s.freeze_transform = v[9]; in.s.trajectory_kind = v[10]; in.s.sampler = v[11];
        in.s.num_tune = v[12]; in.s.maxdepth = v[13]; in.s.store_divergences = v[14]; in.s.store_mass_matrix = v[15];
        in.dev = &facts;
        nm_status st;
        std::string why;
        const EnginePlan p = plan_engine(in, &st, &why);
        if (st != NM_OK) { printf("%s %d refused: %s\n", id, (int)st, why.c_str()); continue; }
        DrawState d;
        d.sampling_from = p.s.num_tune + 1;
        if (v[16]) d.transform = plan_transform(p, v[16] == 2, v[17], in.dim, true);
        std::set<std::string> served;
        const uint64_t cut = v[18], draws = v[19];
        for (int call = 0; call < 2; ++call) {
            d.draws_launched = call ? cut : 0;
            const DrawPlan dp = plan_draw(p, d, call ? draws - cut : cut);
            for (int i = 0; i < dp.n; ++i) {
                switch (dp.step[i].what) {
                    case Launch::Wave: served.insert("wave"); break;
                    case Launch::WaveSampling: served.insert("sampling"); break;
                    case Launch::Group: served.insert("group"); break;
                    case Launch::Lane: served.insert("lane"); break;
                    case Launch::TileDiag: served.insert("tile_diag"); break;
                    case Launch::TilePrec: served.insert("tile"); break;
                    case Launch::Lockstep: served.insert("lockstep"); break;
                }
            }
        }
        printf("%s %d %d %d %d %llu", id, (int)d.transform.status, (int)p.family, p.dpl, p.wpc, (unsigned long long)p.cl_k);
        for (auto& x : served) printf(" %s", x.c_str());
        printf("\n");
    }
    return 0;
}
