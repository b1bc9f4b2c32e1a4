// engine_plan_check.hip — HOST program (compiled with hipcc, runs on the CPU): csrc/engine_plan.hpp's plan_engine / plan_transform /
// plan_draw against expectations written by hand from DESIGN.md's table of kernel families, include/nuts_amd.h's description of
// lane_groups / lane_chains / chain_tiles and the measured crossovers quoted above small_chain_rule — not from the functions' output.
// The device is a constant: 256 compute units, 8 resident blocks per unit of the wave and group kernels (2048 wave slots), 2 of the lane
// kernels.  Exit code 0 and a last line "0 mismatches" = every expectation holds.
#include "../../nuts_rs_amd/csrc/engine_plan.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace nm;
using namespace nm::plan;

static long n_checks = 0, n_bad = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_bad; printf("line %d (%s): %s\n", __LINE__, what.c_str(), #cond); } } while (0)

struct Facts final : DeviceFacts {
    std::string asked;          // the questions in order: r(eady) c(us) w(ave) g(roup) l(ane)
    KernelFamily wave_family = FAMILY_PLAIN, group_family = FAMILY_PLAIN;
    bool lane_kinetic = false;
    bool ready() override { asked += 'r'; return true; }
    bool cu_count(int* cus) override { asked += 'c'; *cus = 256; return true; }
    bool wave_occupancy(KernelFamily f, int, int, int* occ) override { asked += 'w'; wave_family = f; *occ = 8; return true; }
    bool group_occupancy(KernelFamily f, int, int, int* occ) override { asked += 'g'; group_family = f; *occ = 8; return true; }
    bool lane_occupancy(bool kinetic, int* occ) override { asked += 'l'; lane_kinetic = kinetic; *occ = 2; return true; }
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

struct Run { EnginePlan p; nm_status st; std::string why, asked; Facts facts; };
struct Case {
    PlanInput in;
    Case(uint64_t kind, uint64_t dim, uint64_t n_chains) {
        in.s = diag_settings(); in.logp_kind = kind; in.dim = dim; in.n_chains = n_chains;
        memset(&in.cfg, 0, sizeof in.cfg); in.cfg.device = -1;
    }
    Case& lane_groups(uint64_t v) { in.cfg.lane_groups = v; return *this; }
    Case& lane_chains(uint64_t v) { in.cfg.lane_chains = v; return *this; }
    Case& chain_tiles(uint64_t v) { in.cfg.chain_tiles = v; return *this; }
    Case& dims_per_lane(uint64_t v) { in.cfg.dims_per_lane = v; return *this; }
    Case& tune(uint64_t v) { in.s.num_tune = v; return *this; }
    Case& depth(uint64_t maxdepth, uint64_t extra) { in.s.maxdepth = maxdepth; in.s.extra_doublings = extra; return *this; }
    Case& kind(uint64_t v) { in.s.trajectory_kind = v; return *this; }
    Case& mclmc() { in.s.sampler = NM_SAMPLER_MCLMC; return *this; }
    Case& low_rank(bool frozen) { in.s.adaptation = NM_ADAPT_LOW_RANK; in.s.freeze_transform = frozen; return *this; }
    // a module built for (dpl, w): lanes per chain of its group form, lane form, variants
    Case& module(uint64_t dpl, uint64_t w, uint64_t group_lanes, bool lane, uint64_t variants = 0, uint64_t wide = 0) {
        const uint64_t mi[8] = {sizeof(KParams), NM_ABI_VERSION, dpl, w, group_lanes, wide, lane ? 1u : 0u, variants};
        memcpy(in.module.info, mi, sizeof mi);
        in.module.has_launch_lane = lane; in.module.has_launch_variant = variants != 0;
        return *this;
    }
    Run run() {
        Run r;
        in.dev = &r.facts;
        r.p = plan_engine(in, &r.st, &r.why);
        r.asked = r.facts.asked;
        return r;
    }
};

// plan_draw's contract on any engine, from any state: the steps cover the call in order, at most two, and the sampling build never serves
// a draw of the warm-up (index <= num_tune: draw num_tune runs the last adapt transition) or the first draw after a set_position
static void check_draw_contract(const std::string& what, const EnginePlan& p) {
    for (uint64_t set_at : {(uint64_t)0, p.s.num_tune / 2, p.s.num_tune + 3}) {      // the last set_position happened at this draw index
        DrawState d;
        d.sampling_from = set_at == 0 ? p.s.num_tune + 1 : sampling_from_after_set_position(p, set_at);
        for (uint64_t at = set_at; at < p.s.num_tune + 30; ++at)
            for (uint64_t n = 1; n <= 30; ++n) {
                d.draws_launched = at;
                const DrawPlan s = plan_draw(p, d, n);
                uint64_t sum = 0, first = at;
                CHECK(s.n >= 1 && s.n <= 2);
                for (int i = 0; i < s.n; ++i) {
                    CHECK(s.step[i].n_draws > 0 && s.step[i].grid > 0);
                    if (s.step[i].what == Launch::WaveSampling) { CHECK(first > p.s.num_tune); CHECK(set_at == 0 || first > set_at); CHECK(p.sampling_build); }
                    if ((s.step[i].what == Launch::Group || s.step[i].what == Launch::Lane) && !s.step[i].tune) CHECK(first >= p.s.num_tune);
                    first += s.step[i].n_draws; sum += s.step[i].n_draws;
                }
                CHECK(sum == n);
            }
    }
}
static DrawPlan draw(const EnginePlan& p, uint64_t at, uint64_t n, uint64_t sampling_from = 0, TransformPlan t = TransformPlan()) {
    DrawState d;
    d.draws_launched = at; d.sampling_from = sampling_from ? sampling_from : p.s.num_tune + 1; d.transform = t;
    return plan_draw(p, d, n);
}

int main() {
    std::string what;
    // ---- the one-chain-per-lane rule (nuts_amd.h lane_chains: dim <= 4 from 32768 chains, dim <= 10 from 49152, never Neal's funnel) ----
    struct { uint64_t kind, dim, n; bool lane, group; } small[] = {
        {NM_LOGP_IID_NORMAL, 4, 32767, false, true}, {NM_LOGP_IID_NORMAL, 4, 32768, true, false},
        {NM_LOGP_IID_NORMAL, 5, 32768, false, true}, {NM_LOGP_IID_NORMAL, 10, 49151, false, true}, {NM_LOGP_IID_NORMAL, 10, 49152, true, false},
        {NM_LOGP_IID_NORMAL, 11, 65536, false, true}, {NM_LOGP_DIAG_NORMAL, 10, 49152, true, false}, {NM_LOGP_EIGHT_SCHOOLS, 10, 49152, true, false},
        // Neal's funnel: 8 chains per wavefront only for dim <= 16 from 49152 chains on, never one chain per lane
        {NM_LOGP_FUNNEL, 16, 49151, false, false}, {NM_LOGP_FUNNEL, 16, 49152, false, true}, {NM_LOGP_FUNNEL, 17, 49152, false, false}, {NM_LOGP_FUNNEL, 10, 65536, false, true},
        // several chains per wavefront: more chains than wave slots (2048 here)
        {NM_LOGP_IID_NORMAL, 10, 1024, false, false}, {NM_LOGP_IID_NORMAL, 10, 2048, false, false}, {NM_LOGP_IID_NORMAL, 10, 2049, false, true},
        {NM_LOGP_IID_NORMAL, 64, 8192, false, true}, {NM_LOGP_IID_NORMAL, 65, 8192, false, false},
    };
    for (auto& c : small) {
        what = "kind " + std::to_string(c.kind) + " dim " + std::to_string(c.dim) + " x " + std::to_string(c.n);
        Run r = Case(c.kind, c.dim, c.n).run();
        CHECK(r.st == NM_OK);
        CHECK((r.p.lane_grid > 0) == c.lane);
        CHECK((r.p.group_grid > 0) == c.group);
        CHECK(r.p.dpl == 2 && r.p.wpc == 1 && r.p.family == FAMILY_PLAIN && r.p.n_waves == (c.n < 2048 ? c.n : 2048));
        // the same queries in the same cases and order: the group query only once the rule has chosen groups, the lane query likewise
        const bool early = c.lane && c.kind != NM_LOGP_FUNNEL;      // (a lane engine by the automatic rule also has more chains than wave slots: its early group draws)
        CHECK(r.asked == std::string("rwc") + (c.group || early ? "g" : "") + (c.lane ? "l" : ""));
        if (c.lane) CHECK(r.p.lane_grid == 512 && r.p.early_group_grid == 2048);      // min(ceil(n / 64), 2 x 256); the group kernels' grid kept for the first draws
        const Launch first = draw(r.p, 400, 5).step[0].what;      // lane > group > wave, after the warm-up
        CHECK(first == (c.lane ? Launch::Lane : c.group ? Launch::Group : Launch::Wave));
        check_draw_contract(what, r.p);
    }
    {   // group sizes: 8 / 4 / 2 chains per wavefront for dim <= 16 / 32 / 64; the roomy builds for grids of at most 4 x CUs blocks
        what = "group sizes";
        const uint64_t dims[] = {16, 17, 32, 33, 64, 65}, grid64[] = {8, 16, 16, 32, 32, 0};
        for (int i = 0; i < 6; ++i) CHECK(Case(NM_LOGP_IID_NORMAL, dims[i], 64).lane_groups(2).run().p.group_grid == grid64[i]);
        Run roomy = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 8192).run(), tight = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 8193).run();
        CHECK(roomy.p.group_grid == 1024 && roomy.p.group_roomy && tight.p.group_grid == 1025 && !tight.p.group_roomy);
        const DrawPlan a = draw(roomy.p, 0, 500), b = draw(roomy.p, 400, 5), c = draw(tight.p, 399, 5);
        CHECK(a.n == 1 && a.step[0].what == Launch::Group && a.step[0].tune && a.step[0].roomy && a.step[0].grid == 1024);
        CHECK(b.n == 1 && !b.step[0].tune && b.step[0].roomy && c.n == 1 && c.step[0].tune && !c.step[0].roomy);
    }
    {   // the overrides (1 = never, 2 = whenever the kernel applies; lane_chains takes precedence over lane_groups)
        what = "overrides at 64 chains";
        auto P = [](uint64_t g, uint64_t l) { return Case(NM_LOGP_IID_NORMAL, 10, 64).lane_groups(g).lane_chains(l).run().p; };
        CHECK(P(0, 0).group_grid == 0 && P(0, 0).lane_grid == 0);
        CHECK(P(1, 0).group_grid == 0 && P(2, 0).group_grid == 8 && P(2, 0).lane_grid == 0);
        CHECK(P(0, 1).lane_grid == 0 && P(0, 2).lane_grid == 1 && P(0, 2).early_group_grid == 0);
        CHECK(P(2, 2).lane_grid == 1 && P(2, 2).group_grid == 0);
        what = "overrides at 65536 chains";
        CHECK(Case(NM_LOGP_IID_NORMAL, 10, 65536).lane_chains(1).run().p.lane_grid == 0 && Case(NM_LOGP_IID_NORMAL, 10, 65536).lane_chains(1).run().p.group_grid == 2048);
        CHECK(Case(NM_LOGP_IID_NORMAL, 10, 65536).lane_groups(1).run().p.lane_grid == 512 && Case(NM_LOGP_IID_NORMAL, 10, 65536).lane_groups(1).run().p.early_group_grid == 0);
        // the kernels' limits: lane forms up to dim 10 and depth 10, the default tiling only
        CHECK(Case(NM_LOGP_IID_NORMAL, 11, 64).lane_chains(2).run().p.lane_grid == 0);
        CHECK(Case(NM_LOGP_IID_NORMAL, 10, 64).lane_chains(2).lane_groups(2).depth(10, 1).run().p.lane_grid == 0 && Case(NM_LOGP_IID_NORMAL, 10, 64).lane_groups(2).depth(10, 1).run().p.group_grid == 0);
        CHECK(Case(NM_LOGP_IID_NORMAL, 10, 64).lane_chains(2).dims_per_lane(4).run().p.lane_grid == 0);
        CHECK(Case(NM_LOGP_HOST_CALLBACK, 5, 64).lane_chains(2).lane_groups(2).run().p.group_grid == 0);
    }
    {   // 8 schools on a grid that reaches the lane kernels: the first 20 warm-up draws on the group kernels (automatic choice only)
        what = "early group draws";
        Run r = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 49152).tune(30).run();
        const DrawPlan a = draw(r.p, 0, 25), b = draw(r.p, 25, 10), c = draw(r.p, 19, 1), d = draw(r.p, 20, 1), e2 = draw(r.p, 30, 7);
        CHECK(a.n == 2 && a.step[0].what == Launch::Group && a.step[0].n_draws == 20 && a.step[0].tune && !a.step[0].roomy && a.step[0].grid == 2048);
        CHECK(a.step[1].what == Launch::Lane && a.step[1].n_draws == 5 && a.step[1].tune && a.step[1].grid == 512);
        CHECK(b.n == 1 && b.step[0].what == Launch::Lane && b.step[0].n_draws == 10 && b.step[0].tune);
        CHECK(c.n == 1 && c.step[0].what == Launch::Group && d.n == 1 && d.step[0].what == Launch::Lane && e2.n == 1 && !e2.step[0].tune);
        Run s8 = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 49152).tune(8).run();      // a warm-up shorter than 20 draws: group draws end with it
        CHECK(draw(s8.p, 5, 5).step[0].what == Launch::Group && draw(s8.p, 5, 5).n == 1 && draw(s8.p, 8, 5).step[0].what == Launch::Lane && !draw(s8.p, 8, 5).step[0].tune);
        Run f = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 49152).tune(30).lane_chains(2).run();
        CHECK(f.p.early_group_grid == 0 && f.asked == "rwcgl" && draw(f.p, 0, 25).n == 1 && draw(f.p, 0, 25).step[0].what == Launch::Lane);
        check_draw_contract(what, r.p); check_draw_contract(what, s8.p);
    }
    {   // trajectory kinds and MCLMC on a lane-sized count: the kinds have lane forms, MCLMC stays on the groups
        what = "trajectory kinds";
        Run x = Case(NM_LOGP_IID_NORMAL, 10, 49152).kind(NM_TRAJ_EXACT_NORMAL).run(), m = Case(NM_LOGP_IID_NORMAL, 10, 49152).kind(NM_TRAJ_MICROCANONICAL).run();
        Run c = Case(NM_LOGP_IID_NORMAL, 10, 49152).mclmc().run();
        CHECK(x.st == NM_OK && x.p.family == FAMILY_KINETIC && x.p.lane_grid > 0 && x.p.early_group_grid == 0 && x.facts.lane_kinetic && x.facts.wave_family == FAMILY_KINETIC);
        CHECK(m.p.lane_grid > 0 && m.p.family == FAMILY_KINETIC);
        CHECK(c.st == NM_OK && c.p.lane_grid == 0 && c.p.group_grid == 2048 && c.p.family == FAMILY_KINETIC && c.facts.group_family == FAMILY_KINETIC);
        CHECK(c.p.s.step_size_method == NM_STEP_FIXED && c.p.s.fixed_step_size == 0.5 && c.p.s.trajectory_kind == NM_TRAJ_EUCLIDEAN);      // the normalised settings
        CHECK(!Case(NM_LOGP_IID_NORMAL, 300, 8).kind(NM_TRAJ_EXACT_NORMAL).run().p.sampling_build);
    }
    {   // the full-precision normal, per-chain diagonal adaptation: the matrix cores from 256 chains on (beyond 32 dims: up to there the group
        // kernels are faster, tools/probes/mvn_small_dims.py), dim <= 256; chain_tiles 1 = never, 2 = whenever it applies
        what = "mvn tile diag";
        struct { uint64_t dim, n, tiles; bool tile; int dpl; } mv[] = {
            {32, 255, 0, false, 2}, {32, 256, 0, false, 2}, {33, 255, 0, false, 2}, {33, 256, 0, true, 4}, {128, 255, 0, false, 2}, {128, 256, 0, true, 4},
            {129, 255, 0, false, 4}, {129, 256, 0, true, 4}, {256, 256, 0, true, 4}, {257, 256, 0, false, 8},
            {64, 256, 1, false, 2}, {64, 255, 2, true, 4}, {16, 64, 2, true, 4},
        };
        for (auto& c : mv) {
            what = "mvn dim " + std::to_string(c.dim) + " x " + std::to_string(c.n) + " chain_tiles " + std::to_string(c.tiles);
            Run r = Case(NM_LOGP_MVN_PREC, c.dim, c.n).chain_tiles(c.tiles).run();
            CHECK(r.st == NM_OK && r.p.tile_diag == c.tile && r.p.dpl == c.dpl && r.p.wpc == 1 && r.p.group_grid == 0 && r.p.lane_grid == 0);
            CHECK(draw(r.p, 0, 3).n == 1 && draw(r.p, 0, 3).step[0].what == (c.tile ? Launch::TileDiag : Launch::Wave));
            if (c.tile) CHECK(draw(r.p, 0, 3).step[0].grid == (c.n + 15) / 16 && r.p.scratch_slots >= 16u * r.p.tile_grid);
            check_draw_contract(what, r.p);
        }
        what = "group > tile diag > wave";
        Run g = Case(NM_LOGP_MVN_PREC, 64, 256).lane_groups(2).run();
        CHECK(g.p.group_grid == 128 && !g.p.tile_diag && g.p.dpl == 2 && draw(g.p, 0, 3).step[0].what == Launch::Group);
        CHECK(!Case(NM_LOGP_MVN_PREC, 64, 256).kind(NM_TRAJ_EXACT_NORMAL).run().p.tile_diag);
    }
    {   // one frozen low-rank transformation for all chains (chain_tiles: 0 = the lockstep kernel where it applies, else the tile kernel;
        // 2 = always the tile kernel; 3 = the lockstep kernel or an error)
        what = "shared frozen transformation";
        auto E = [](uint64_t dim, uint64_t tiles) { return Case(NM_LOGP_MVN_PREC, dim, 32).low_rank(true).tune(4).depth(3, 0).chain_tiles(tiles); };
        Run a = E(64, 0).run();
        CHECK(a.st == NM_OK && a.p.family == FAMILY_LOW_RANK && a.p.dpl == 4 && a.p.lr_rmax == 64 && a.p.lr_cap == 6 && !a.p.sampling_build && a.asked == "rwc");
        TransformPlan t = plan_transform(a.p, false, 8, 64, true);
        CHECK(t.tile && t.lock && t.status == NM_OK);
        CHECK(draw(a.p, 0, 3, 0, t).n == 1 && draw(a.p, 0, 3, 0, t).step[0].what == Launch::Lockstep && draw(a.p, 0, 3, 0, t).step[0].grid == 2);
        CHECK(draw(a.p, 0, 3).step[0].what == Launch::Wave);      // before any set_transform
        // a later call that does not qualify: rank no multiple of 8, per-chain, refused input — neither kernel, no error when automatic
        for (TransformPlan u : {plan_transform(a.p, false, 4, 64, true), plan_transform(a.p, true, 8, 64, true), plan_transform(a.p, false, 8, 64, false)})
            CHECK(!u.tile && !u.lock && u.status == NM_OK);
        Case sd = E(64, 0); sd.in.s.store_divergences = 1;
        Case sm = E(64, 0); sm.in.s.store_mass_matrix = 1;
        for (Case* c : {&sd, &sm}) { t = plan_transform(c->run().p, false, 8, 64, true); CHECK(t.tile && !t.lock && t.status == NM_OK); }
        t = plan_transform(E(64, 1).run().p, false, 8, 64, true);
        CHECK(!t.tile && !t.lock && E(64, 1).run().p.dpl == 2);
        t = plan_transform(E(16, 2).run().p, false, 8, 16, true);
        CHECK(t.tile && !t.lock && t.status == NM_OK && draw(E(16, 2).run().p, 0, 3, 0, t).step[0].what == Launch::TilePrec);
        t = plan_transform(E(16, 3).run().p, false, 8, 16, true);
        CHECK(t.tile && t.lock && t.status == NM_OK);
        t = plan_transform(E(16, 3).depth(6, 6).run().p, false, 8, 16, true);      // maxdepth + extra_doublings = 12: an error, the tile kernel stands
        CHECK(t.tile && !t.lock && t.status == NM_ERR_UNSUPPORTED);
        t = plan_transform(E(64, 0).depth(6, 6).run().p, false, 8, 64, true);
        CHECK(t.tile && !t.lock && t.status == NM_OK);
        t = plan_transform(E(16, 3).run().p, false, 4, 16, true);
        CHECK(!t.tile && !t.lock && t.status == NM_ERR_UNSUPPORTED);
        CHECK(Case(NM_LOGP_MVN_PREC, 64, 32).low_rank(false).run().p.dpl == 2);      // a per-chain adapting run keeps its lanes busy
    }
    {   // the sampling build: tilings (8,1) (16,1) of the plain iid / diagonal / funnel / full-precision normal kernels, layouts up to 12 levels
        what = "sampling build";
        Run r = Case(NM_LOGP_IID_NORMAL, 300, 8).tune(3).depth(3, 0).run();
        CHECK(r.st == NM_OK && r.p.dpl == 8 && r.p.wpc == 1 && r.p.sampling_build && r.p.n_waves == 8);
        const DrawPlan a = draw(r.p, 0, 2), b = draw(r.p, 2, 4), c = draw(r.p, 6, 3, sampling_from_after_set_position(r.p, 6)), d = draw(r.p, 4, 1), e2 = draw(r.p, 3, 1);
        CHECK(a.n == 1 && a.step[0].what == Launch::Wave && a.step[0].n_draws == 2);
        CHECK(b.n == 2 && b.step[0].what == Launch::Wave && b.step[0].n_draws == 2 && b.step[1].what == Launch::WaveSampling && b.step[1].n_draws == 2 && b.step[1].grid == 8);
        CHECK(c.n == 2 && c.step[0].what == Launch::Wave && c.step[0].n_draws == 1 && c.step[1].what == Launch::WaveSampling && c.step[1].n_draws == 2);
        CHECK(d.n == 1 && d.step[0].what == Launch::WaveSampling && e2.n == 1 && e2.step[0].what == Launch::Wave);
        check_draw_contract(what, r.p);
        CHECK(Case(NM_LOGP_IID_NORMAL, 300, 8).depth(3, 9).run().p.sampling_build && !Case(NM_LOGP_IID_NORMAL, 300, 8).depth(3, 10).run().p.sampling_build);
        CHECK(!Case(NM_LOGP_EIGHT_SCHOOLS, 10, 8).run().p.sampling_build && !Case(NM_LOGP_IID_NORMAL, 200, 8).run().p.sampling_build);
        CHECK(Case(NM_LOGP_IID_NORMAL, 1024, 8).run().p.sampling_build && !Case(NM_LOGP_IID_NORMAL, 1025, 8).run().p.sampling_build);
        CHECK(Case(NM_LOGP_FUNNEL, 300, 8).run().p.sampling_build && Case(NM_LOGP_MVN_PREC, 300, 8).run().p.sampling_build && !Case(NM_LOGP_HOST_CALLBACK, 300, 8).run().p.sampling_build);
        Run n = Case(NM_LOGP_EIGHT_SCHOOLS, 10, 8).tune(3).run();
        CHECK(draw(n.p, 2, 4).n == 1 && draw(n.p, 2, 4).step[0].what == Launch::Wave);
    }
    {   // chains wider than one block, a host callback, user modules
        what = "wide chains";
        Run w = Case(NM_LOGP_DIAG_NORMAL, 4097, 8).run();
        CHECK(w.st == NM_OK && w.p.family == FAMILY_CLUSTER && w.p.cl_k == 2 && w.p.dpl == 16 && w.p.wpc == 4 && w.p.n_waves == 16 && w.p.n_clusters == 8 && w.asked == "rwc");
        CHECK(Case(NM_LOGP_IID_NORMAL, 4097, 8).kind(NM_TRAJ_MICROCANONICAL).run().p.family == FAMILY_CLUSTER_KINETIC);
        CHECK(Case(NM_LOGP_IID_NORMAL, 131072, 8).run().st == NM_OK && Case(NM_LOGP_IID_NORMAL, 131072, 8).run().p.cl_k == 32);
        what = "host callback";
        Run h = Case(NM_LOGP_HOST_CALLBACK, 5, 4096).lane_groups(2).lane_chains(2).run();
        CHECK(h.st == NM_OK && h.p.group_grid == 0 && h.p.lane_grid == 0 && h.p.n_waves == 2048 && draw(h.p, 0, 3).step[0].what == Launch::Wave);
        what = "modules";
        Run plain = Case(NM_LOGP_MODULE, 40, 64).module(2, 1, 0, false).lane_groups(2).run();
        CHECK(plain.st == NM_OK && plain.p.group_grid == 0 && plain.asked == "rwc");
        Run grp = Case(NM_LOGP_MODULE, 10, 64).module(2, 1, 8, false).lane_groups(2).run();
        CHECK(grp.st == NM_OK && grp.p.group_grid == 8 && !grp.p.group_roomy);      // (the roomy builds: built-in densities)
        CHECK(Case(NM_LOGP_MODULE, 10, 64).module(2, 1, 8, false).lane_chains(2).run().p.lane_grid == 0);
        Run ln = Case(NM_LOGP_MODULE, 10, 64).module(2, 1, 8, true).lane_chains(2).run();
        CHECK(ln.st == NM_OK && ln.p.lane_grid == 1 && ln.asked == "rwcl");
        Run big = Case(NM_LOGP_MODULE, 10, 49152).module(2, 1, 8, true).run();
        CHECK(big.p.lane_grid == 512 && big.p.early_group_grid == 0);      // (the early group draws: built-in densities)
        CHECK(Case(NM_LOGP_MODULE, 20, 64).module(2, 1, 8, false).lane_groups(2).run().p.group_grid == 0);      // a group form of another size
    }
    {   // refusals, each with its status, none of which reaches the device
        what = "refusals";
        struct { Case c; nm_status st; } no[] = {
            {Case(NM_LOGP_IID_NORMAL, 131073, 8), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 4097, 8).low_rank(false), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_FUNNEL, 4097, 8), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 4097, 8).dims_per_lane(8), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 10, 64).lane_chains(3), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 300, 8).dims_per_lane(2), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 10, 8).depth(15, 6), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_IID_NORMAL, 10, 8).kind(3), NM_ERR_INVALID_ARG},
            {Case(NM_LOGP_IID_NORMAL, 1, 8).mclmc(), NM_ERR_INVALID_ARG},
            {Case(NM_LOGP_IID_NORMAL, 1, 8).kind(NM_TRAJ_MICROCANONICAL), NM_ERR_INVALID_ARG},
            {Case(NM_LOGP_IID_NORMAL, 10, 8).tune(0), NM_ERR_INVALID_ARG},
        };
        for (auto& c : no) { Run r = c.c.run(); CHECK(r.st == c.st && !r.why.empty() && r.asked.empty()); }
        Case j(NM_LOGP_IID_NORMAL, 10, 8); j.in.s.early_window = 1.0;
        CHECK(j.run().st == NM_ERR_INVALID_ARG);
        // a module's facts are checked once the device is there, before any kernel is asked
        struct { Case c; nm_status st; } mod[] = {
            {Case(NM_LOGP_MODULE, 40, 8).module(4, 1, 0, false), NM_ERR_INVALID_ARG},                  // another tiling
            {Case(NM_LOGP_MODULE, 40, 8).module(2, 1, 0, false).low_rank(false), NM_ERR_UNSUPPORTED},  // no low-rank kernels
            {Case(NM_LOGP_MODULE, 40, 8).module(2, 1, 0, false).kind(NM_TRAJ_EXACT_NORMAL), NM_ERR_UNSUPPORTED},
            {Case(NM_LOGP_MODULE, 40, 8).module(2, 1, 0, false, 0, 1), NM_ERR_INVALID_ARG},            // built for wide chains
            {Case(NM_LOGP_MODULE, 4097, 8).module(16, 4, 0, false), NM_ERR_INVALID_ARG},               // not built for wide chains
        };
        for (auto& c : mod) { Run r = c.c.run(); CHECK(r.st == c.st && !r.why.empty() && r.asked == "r"); }
        Case abi = Case(NM_LOGP_MODULE, 40, 8).module(2, 1, 0, false); abi.in.module.info[1] += 1;
        CHECK(abi.run().st == NM_ERR_INVALID_ARG);
        CHECK(Case(NM_LOGP_MODULE, 40, 8).module(2, 1, 0, false, 1).low_rank(false).run().st == NM_OK);
        // the device holds too few blocks for a chain of 32
        Case few(NM_LOGP_IID_NORMAL, 131072, 8); few.in.cfg.grid_blocks = 255;
        CHECK(few.run().st == NM_ERR_UNSUPPORTED && few.run().asked == "rwc");
    }
    printf("%ld checks\n%ld mismatches\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
