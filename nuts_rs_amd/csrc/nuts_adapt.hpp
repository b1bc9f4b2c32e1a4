// The chain's scalar step-size protocol: what stepsize::Strategy and GlobalStrategy::adapt (reference src/stepsize/adapt.rs,
// src/stepsize/dual_avg.rs, src/stepsize/adam.rs, src/adapt_strategy.rs:121-222) do to the per-chain scalars, as templates over a math
// policy M — a struct with static exp(double) and log(double) built from a kernel family's own forms of the restated exp / ln, which all
// return the same bits.  Used by the one-chain-per-lane kernels (nuts_lane.hpp, LMath: lexp / llog) and by the lockstep kernel
// (nuts_lockstep.hpp, LMath too).  The one-chain-per-wavefront kernels (nuts_kernels.hpp: stepsize_adapt_reset, update_estimator,
// update_stepsize, adapt, adapt_lr) and the several-lanes-per-chain kernels (nuts_group_impl.hpp: g_*) keep their own statements of the
// same lines: moved here, their warm-up code was re-scheduled and measured 0.3 - 0.6 % slower (DESIGN §1,
// profiles/r12_adapt_dedupe_ab.txt).  A change to the protocol is made here and in those two.  The vector halves of `adapt` (estimator
// loads and stores, the mass-matrix update) and stepsize_init stay with each family.
//
// Included by nuts_kernels.hpp once ChainScalars, KParams and powi_rs exist; the other families see it through that include.  The oracle
// (oracle/nmo_nuts.hpp) is the independent restatement and does not include it.
#pragma once

namespace nm {

// DualAverage::new (dual_avg.rs:44-53) or Adam::new (adam.rs:56-64), as stepsize::Strategy::{new, init} pick them
template <class M>
NM_DEV void stepsize_adapt_reset(ChainScalars& sc, const nm_settings& s, double initial_step) {
    sc.log_step = M::log(initial_step);
    if (s.step_size_method == NM_STEP_ADAM) {
        sc.adam_m = 0.; sc.adam_v = 0.; sc.adam_t = 0;
        return;
    }
    sc.log_step_adapted = sc.log_step;
    sc.hbar = 0.;
    sc.mu = M::log(10. * initial_step);
    sc.da_count = 1;
}

// DualAverage::advance (reference src/stepsize/dual_avg.rs:55-64) / Adam::advance (stepsize/adam.rs:70-98)
template <class M>
NM_DEV void update_estimator(ChainScalars& sc, const KParams& P, bool late) {
    const nm_settings& s = P.s;
    if (s.step_size_method == NM_STEP_FIXED) return;
    const double accept_stat = late ? sc.last_sym_mean_tree_accept : sc.last_mean_tree_accept;
    if (s.step_size_method == NM_STEP_ADAM) {
        const double gradient = accept_stat - s.target_accept;
        sc.adam_t += 1;
        sc.adam_m = s.adam_beta1 * sc.adam_m + (1.0 - s.adam_beta1) * gradient;
        sc.adam_v = s.adam_beta2 * sc.adam_v + (1.0 - s.adam_beta2) * gradient * gradient;
        const double m_hat = sc.adam_m / (1.0 - powi_rs(s.adam_beta1, (int32_t)sc.adam_t));
        const double v_hat = sc.adam_v / (1.0 - powi_rs(s.adam_beta2, (int32_t)sc.adam_t));
        sc.log_step += s.adam_learning_rate * m_hat / (__builtin_sqrt(v_hat) + s.adam_epsilon);
        return;
    }
    const double w = 1. / ((double)sc.da_count + s.da_t0);
    sc.hbar = (1. - w) * sc.hbar + w * (s.target_accept - accept_stat);
    sc.log_step = sc.mu - sc.hbar * __builtin_sqrt((double)sc.da_count) / s.da_gamma;
    sc.log_step = fmin_rs(sc.log_step, P.ln_max_step);
    const double mk = M::exp(-s.da_k * M::log((double)sc.da_count));
    sc.log_step_adapted = mk * sc.log_step + (1. - mk) * sc.log_step_adapted;
    sc.da_count += 1;
}

// update_stepsize (reference src/stepsize/adapt.rs:235-267); `rng` is the chain's generator (the jitter draw is its next u64)
template <class M, class Rng>
NM_DEV void update_stepsize(ChainScalars& sc, const KParams& P, Rng& rng, bool use_best_guess) {
    const nm_settings& s = P.s;
    const double step = s.step_size_method == NM_STEP_FIXED ? s.fixed_step_size
                      : s.step_size_method == NM_STEP_ADAM ? M::exp(sc.log_step)          // Adam has no averaged iterate
                      : (use_best_guess ? M::exp(sc.log_step_adapted) : M::exp(sc.log_step));
    if (s.has_jitter) {
        const double v12 = u2d((rng.next_u64() >> 12) | 0x3ff0000000000000ull);
        const double j = (v12 - 1.0) * P.jitter_scale + P.jitter_low;
        sc.step_size = step * j;
    } else {
        sc.step_size = step;
    }
}

// the size of the window after the current one (adapt_strategy.rs:167-174)
NM_DEV uint64_t next_window_size(const ChainScalars& sc, const nm_settings& s, bool is_early) {
    if (is_early) return s.early_mass_matrix_switch_freq;
    // (current_window_size as f64 * growth).round() as u64 : round half away from zero
    const double gv = (double)sc.current_window_size * s.mass_matrix_window_growth;
    const double fl = __builtin_floor(gv);
    const uint64_t grown = (uint64_t)((gv - fl >= 0.5) ? fl + 1.0 : fl);
    return sc.current_window_size + 1 > grown ? sc.current_window_size + 1 : grown;
}

// step_size.update (stepsize/adapt.rs:201-209): what the draw's acceptance collector saw
template <class Collector>
NM_DEV void record_collector(ChainScalars& sc, Collector& col) {
    sc.last_mean_tree_accept = col.mean();
    sc.last_sym_mean_tree_accept = col.mean_sym();
    sc.last_n_steps = col.count;
    sc.last_max_energy_error = col.max_energy_error;
}

// step_size_bar of the statistics row (extract_stats, stepsize/adapt.rs:287-299)
template <class M>
NM_DEV double step_size_bar(const ChainScalars& sc, const nm_settings& s) {
    return s.step_size_method == NM_STEP_FIXED ? s.fixed_step_size
         : s.step_size_method == NM_STEP_ADAM ? M::exp(sc.log_step) : M::exp(sc.log_step_adapted);
}

}  // namespace nm
