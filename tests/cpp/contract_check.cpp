// contract_check.cpp — what host code and kernels agree on (csrc/nuts_contract.hpp), printed one fact per line as `name value`.
// A plain host compiler builds it: the header stands alone.  tests/test_contract_header.py compares the lines with
// tests/golden/host_kernel_contract_parent.json, recorded from this program text against the kernel headers of the commit before the
// facts moved (NM_CONTRACT_CHECK_PART 1: a plain unit's facts, 2: those only a tile-mode unit could name then; 0, the default: all).
#include "../../nuts_rs_amd/csrc/nuts_contract.hpp"
#include <cstddef>
#include <cstdio>

#ifndef NM_CONTRACT_CHECK_PART
#define NM_CONTRACT_CHECK_PART 0
#endif

using namespace nm;

#define SIZE(T) printf("sizeof(" #T ") %zu\n", sizeof(T))
#define OFF(T, m) printf("offsetof(" #T "," #m ") %zu\n", offsetof(T, m))
#define VAL(x) printf(#x " %lld\n", (long long)(x))

int main() {
#if NM_CONTRACT_CHECK_PART != 2
    SIZE(KParams); SIZE(ChainScalars); SIZE(lane::LaneParams); SIZE(CbMail);
#define K(m) OFF(KParams, m)
    K(s); K(n_chains); K(dim); K(dpad); K(chain_id_offset); K(nsslot); K(pvec); K(svec); K(sc); K(zig_x); K(zig_f); K(logp_params);
    K(early_end); K(final_step_size_window); K(mclmc_switch_draw); K(cl_k); K(cl_slice); K(cl_general); K(cl_box); K(cl_cnt);
    K(ln_max_step); K(jitter_low); K(jitter_scale); K(out_positions); K(out_stats); K(out_gradient); K(out_tpos); K(out_tgrad);
    K(out_mm_inv); K(out_mm_mu); K(out_div_start); K(out_div_start_grad); K(out_div_end); K(n_draws); K(prof); K(x0); K(lrvec);
    K(lrval); K(lrwin); K(lr_rmax); K(lr_cap); K(draw_end); K(row_base); K(out_mm_eigvals); K(init_mask); K(cb_mail); K(cb_stride);
    K(layout_md);
#undef K
#define C(m) OFF(ChainScalars, m)
    C(key); C(rng_pos); C(logp); C(logdet); C(transform_id); C(mm_logdet); C(mm_id); C(step_size); C(draw_count); C(last_update);
    C(current_window_size); C(tuning); C(has_initial_mass_matrix); C(cnt_fg); C(cnt_bg); C(log_step); C(log_step_adapted); C(hbar);
    C(mu); C(da_count); C(adam_m); C(adam_v); C(adam_t); C(last_mean_tree_accept); C(last_sym_mean_tree_accept);
    C(last_max_energy_error); C(last_n_steps); C(status); C(total_steps); C(px_stale); C(stats_last_id); C(lr_has_inner); C(lr_rank);
    C(lr_start); C(lr_len); C(lr_split); C(lr_pending); C(lr_upd_ok); C(lr_upd_rank); C(lr_upd_logdet); C(lr_is_late); C(lr_row);
    C(kin);
#undef C
    VAL(K_INIT); VAL(K_DRAW); VAL(K_QUERY); VAL(K_GROUP_DRAW); VAL(K_GROUP_TUNE); VAL(K_GROUP_QUERY); VAL(K_GROUP_DRAW_ROOMY);
    VAL(K_GROUP_TUNE_ROOMY); VAL(K_DRAW_SAMPLING);
    for (int k = K_INIT; k <= K_DRAW_SAMPLING; ++k) printf("is_group_kind(%d) %d\n", k, (int)is_group_kind((KernelKind)k));
    VAL(P_X); VAL(P_GX); VAL(P_Z); VAL(P_GZ); VAL(P_SIG); VAL(P_ISIG); VAL(P_MU); VAL(E_DM); VAL(E_DV); VAL(E_GM); VAL(E_GV);
    VAL(B_DM); VAL(B_DV); VAL(B_GM); VAL(B_GV); VAL(P_V); VAL(NUM_PSLOT);
    VAL(EDGE0_Z); VAL(EDGE0_V); VAL(EDGE0_G); VAL(EDGE1_Z); VAL(EDGE1_V); VAL(EDGE1_G); VAL(EDGE2_Z); VAL(EDGE2_V); VAL(EDGE2_G);
    VAL(STAGE_V); VAL(S_DYN);
    VAL(LR_IDLE); VAL(LR_WAIT_HOST); VAL(LR_ANSWERED); VAL(LR_SET_TRANSFORM);
    VAL(MAX_MAXDEPTH); VAL(NM_RING); VAL(NM_BATCH_MAX_DPL); VAL(CL_MAX_MEMBERS); VAL(NM_MF_MAX_MD); VAL(grp::GMAXDEPTH);
    VAL(lane::LMAXDEPTH);
    for (int d = 0; d <= 65; ++d) printf("group_size(%d) %d\n", d, grp::group_size((uint64_t)d));
    for (int d = 0; d <= 17; ++d) printf("lane_pairs(%d) %d\n", d, lane::lane_pairs((uint64_t)d));
    for (int md = 0; md <= 20; ++md) printf("num_sslots(%d) %d\n", md, num_sslots(md));
    for (int id = 0; id <= 2; ++id) printf("slot_edge(%d) %d\n", id, slot_edge(id));
    printf("slot_F(0) %d\n", slot_F(0));
    for (int md = 10; md <= 20; md += 10) {
        printf("slot_F(%d) %d\n", md, slot_F(md));
        printf("slot_L(%d,0) %d\nslot_L(%d,%d) %d\n", md, slot_L(md, 0), md, md, slot_L(md, md));
        printf("slot_C(%d,0) %d\nslot_C(%d,%d) %d\n", md, slot_C(md, 0), md, md + 2, slot_C(md, md + 2));
        printf("slot_R(%d,0) %d\nslot_R(%d,%d) %d\n", md, slot_R(md, 0), md, NM_RING - 1, slot_R(md, NM_RING - 1));
    }
    {
        nm_settings s = {};
        s.maxdepth = 10; s.extra_doublings = 2;
        printf("layout_depth(10+2) %d\n", layout_depth(s));
    }
    static const int tilings[8][2] = {{2, 1}, {4, 1}, {8, 1}, {16, 1}, {8, 2}, {16, 2}, {4, 4}, {16, 4}};   // {doubles per lane, waves per chain}
    for (auto& t : tilings) {
        for (int plain = 0; plain <= 1; ++plain) printf("batched_merges(%d,%d,%d) %d\n", t[0], t[1], plain, (int)batched_merges(t[0], t[1], plain != 0));
        printf("sampling_tiling(%d,%d) %d\n", t[0], t[1], (int)sampling_tiling(t[0], t[1]));
    }
    VAL(NM_LOGP_IID_NORMAL); VAL(NM_LOGP_DIAG_NORMAL); VAL(NM_LOGP_FUNNEL); VAL(NM_LOGP_EIGHT_SCHOOLS); VAL(NM_LOGP_MVN_PREC);
    VAL(NM_LOGP_MODULE); VAL(NM_LOGP_HOST_CALLBACK);
    for (uint64_t kind = NM_LOGP_IID_NORMAL; kind <= NM_LOGP_HOST_CALLBACK; ++kind) printf("sampling_logp_kind(%d) %d\n", (int)kind, (int)sampling_logp_kind(kind));
#endif
#if NM_CONTRACT_CHECK_PART != 1
    SIZE(tile::TileMats);
#define T(m) OFF(tile::TileMats, m)
    T(ut); T(u); T(p); T(dim); T(rank); T(dim_kp); T(rank_kp); T(dim_st); T(rank_st);
#undef T
    VAL(NM_TILE_CHAINS); VAL(NM_TILE_OCC); VAL(lock::LOCK_MAXDEPTH);
#endif
    return 0;
}
