// merge_filter_check.hip — HOST program (compiled with hipcc, runs on the CPU): the sampling build's merge filter (csrc/dev_math.hpp
// merge_filter_impl, round 10) against the exact procedure merge_math_impl.
//   (a) soundness: wherever the filter answers "decided" on operands perturbed by up to +-NM_MF_EPS_MAX, its flags are the exact procedure's on the
//       unperturbed pair and fatal is not among them (>= 1e7 random cases and a grid of special operands and words);
//   (b) the error bounds the derivation uses, measured: mf_exp and mf_log1p(mf_exp(.)) against exp_sl / log1p_unit on EVERY f32 in [-40, 0];
//   (c) whole trees (>= 1e5, 1 .. 10 doublings, four laws of leaf weights, discarded doublings): approximate track + filter + leaf log + replay
//       against the all-exact procedure: every flag triple, the words consumed, every node's |L~ - L| <= NM_MF_EPS_MAX, every replayed operand's bits;
//   and the undecided share on uniform words, |a - b| <= 5, without the forced 1 in 2^NM_MF_FORCE_BITS: at most 4 kappa.
// Prints "... 0 mismatches"; exit code 0 = all of it holds.
#include "../../nuts_rs_amd/csrc/dev_math.hpp"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <thread>
#include <vector>
using namespace nm;
struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    double unif() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = 1.0 - unif(), v = unif(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};
static long bad = 0;
static const double EPS = NM_MF_EPS_MAX;
static const double KAPPA = (double)NM_MF_KAPPA;

// x + delta, no further from x than EPS after rounding
static double perturb(double x, double delta) {
    double y = x + delta;
    if (std::fabs(y - x) > EPS) y = std::nextafter(y, x);
    return y;
}
static long n_sound = 0, n_decided = 0;
static void sound(double a, double b, uint32_t is_main, uint64_t w, double da, double db) {
    const MergeOut r = merge_math_impl(a, b, is_main, (uint32_t)w, (uint32_t)(w >> 32));
    const MergeOut f = merge_filter_impl(perturb(a, da), perturb(b, db), is_main, (uint32_t)w, (uint32_t)(w >> 32));
    n_sound++;
    if (f.flags == NM_MF_UNDECIDED) return;
    n_decided++;
    if (f.flags != r.flags || (f.flags & 4u) || (f.flags & ~7u)) {
        if (bad++ < 20) printf("soundness: a %a b %a (+%g, +%g) main %u w %016llx: filter flags %u, exact %u\n", a, b, da, db, is_main, (unsigned long long)w, f.flags, r.flags);
    }
}
static void sound_all(double a, double b, uint32_t is_main, uint64_t w) {
    for (double da : {-EPS, 0.0, EPS}) for (double db : {-EPS, 0.0, EPS}) sound(a, b, is_main, w, da, db);
}
// the exact procedure's p of a pair (what the Bernoulli word is compared with)
static double exact_p(double a, double b, uint32_t is_main) {
    const double self = is_main ? a : logaddexp_sl(a, b);
    return exp_sl(b - self);
}
static uint64_t word_at(double p, double rel, int64_t off) {
    const double t = p * (1.0 + rel) * 18446744073709551616.0;
    if (!(t >= 0.0)) return 0;
    if (t >= 18446744073709549568.0) return ~0ull;
    return (uint64_t)t + (uint64_t)off;
}

// (b) every f32 in [-40, 0]
static void sweep(uint32_t lo, uint32_t hi, double* max_e, double* max_s, long* out_of_range) {
    double me = 0., ms = 0.;
    long oor = 0;
    for (uint32_t u = lo; u < hi; ++u) {
        float x;
        const uint32_t bits = 0x80000000u | u;
        memcpy(&x, &bits, 4);
        const float e = mf_exp(x);
        const double ex = exp_sl((double)x);
        const double re = std::fabs((double)e / ex - 1.0);
        const double se = std::fabs((double)mf_log1p(e) - log1p_unit(ex));
        if (!(e > 0.0f && e <= 1.0f)) oor++;
        if (!(re <= me)) me = re;
        if (!(se <= ms)) ms = se;
    }
    *max_e = me; *max_s = ms; *out_of_range = oor;
}

// (c) one tree: `depth` doublings, a doubling discarded now and then (its leaves overwritten in the log by the next one at its depth)
struct TreeStats { long merges = 0, replays = 0, words = 0; double max_err = 0.; };
static bool run_tree(Rng& g, int depth, int law, TreeStats& ts) {
    std::vector<double> log((size_t)1 << depth, 0.0);
    std::vector<uint64_t> words;
    const double c_eq = g.normal() * 3.0;
    auto leaf = [&]() {
        switch (law) {
        case 0: return g.normal() * 0.1;
        case 1: return g.normal() * 3.0;
        case 2: { const double u = g.unif(); return u < 0.02 ? 500.0 : (u < 0.04 ? -500.0 : g.normal() * 0.5); }
        default: return c_eq;
        }
    };
    size_t pos_x = 0, pos_a = 0;                 // words consumed by the exact / the approximate track
    auto word = [&](size_t pos) { while (words.size() <= pos) words.push_back(g.next()); return words[pos]; };
    // one merge on both tracks; (first, count) as the kernel passes them.  Returns false on a mismatch.
    auto merge = [&](double ax, double bx, double aa, double ba, uint32_t is_main, uint32_t first, uint32_t count, double& tx, double& ta, bool& take) {
        const uint64_t wx = word(pos_x), wa = word(pos_a);
        const MergeOut r = merge_math_impl(ax, bx, is_main, (uint32_t)wx, (uint32_t)(wx >> 32));
        MergeOut f = merge_filter_impl(aa, ba, is_main, (uint32_t)wa, (uint32_t)(wa >> 32));
        ts.merges++;
        if (f.flags & NM_MF_UNDECIDED) {
            ts.replays++;
            const double a = is_main ? mf_fold_main(log.data(), (uint32_t)__builtin_ctz(count)) : mf_fold(log.data(), first, count);
            const double b = is_main ? mf_fold(log.data(), count - 1u, count) : mf_fold(log.data(), first + count, count);
            if (d2u(a) != d2u(ax) || d2u(b) != d2u(bx)) { if (bad++ < 20) printf("replay: (%a, %a) is not the exact track's (%a, %a), first %u count %u main %u\n", a, b, ax, bx, first, count, is_main); return false; }
            f = is_main ? merge_math_main_impl(a, b, (uint32_t)wa, (uint32_t)(wa >> 32)) : merge_math_impl(a, b, 0u, (uint32_t)wa, (uint32_t)(wa >> 32));
            if (d2u(f.total) != d2u(r.total)) { if (bad++ < 20) printf("replay: total %a, exact track %a\n", f.total, r.total); return false; }
        }
        if (f.flags != r.flags) { if (bad++ < 20) printf("tree: flags %u, exact %u at (%a, %a) ~ (%a, %a) main %u\n", f.flags, r.flags, ax, bx, aa, ba, is_main); return false; }
        const double err = std::fabs(f.total - r.total);
        if (!(err <= EPS) && !(f.total == r.total)) { if (bad++ < 20) printf("tree: |L~ - L| = %g at (%a, %a) main %u\n", err, ax, bx, is_main); return false; }
        if (err > ts.max_err) ts.max_err = err;
        pos_x += (r.flags & 2u) ? 1 : 0; pos_a += (f.flags & 2u) ? 1 : 0;
        tx = r.total; ta = f.total; take = (r.flags & 1u) != 0;
        return true;
    };
    double main_x = 0.0, main_a = 0.0;
    for (int d = 0; d < depth;) {
        const uint32_t nleaf = 1u << d, base = nleaf - 1u;
        const bool discard = g.unif() < 0.1;
        const uint32_t stop_at = discard ? (uint32_t)(g.next() % nleaf) | 1u : nleaf;      // discarded after the merges of this (odd) leaf, as a U-turn below the top does
        double sub_x = 0., sub_a = 0.;
        bool take;
        if (d == 0) { log[0] = leaf(); sub_x = sub_a = log[0]; if (discard) continue; }
        else {
            double px[NM_MF_MAX_MD + 1], pa[NM_MF_MAX_MD + 1];
            bool ended = false;
            for (uint32_t n = 0; n < nleaf && !ended; n += 2) {
                const double we = leaf(), wo = leaf();
                log[base + n] = we; log[base + n + 1] = wo;
                const uint32_t nn = n + 1;
                const int t = __builtin_ctz(~nn);
                if (!merge(we, wo, we, wo, 0u, base + n, 1u, sub_x, sub_a, take)) return false;
                for (int k = 2; k <= t; ++k)
                    if (!merge(px[k - 1], sub_x, pa[k - 1], sub_a, 0u, nleaf + nn - (1u << k), 1u << (k - 1), sub_x, sub_a, take)) return false;
                px[t] = sub_x; pa[t] = sub_a;
                if (nn >= stop_at) ended = true;
            }
            if (ended && discard) continue;
        }
        if (!merge(main_x, sub_x, main_a, sub_a, 1u, 0u, nleaf, main_x, main_a, take)) return false;
        d += 1;
    }
    if (pos_x != pos_a) { if (bad++ < 20) printf("tree: %zu words consumed, exact %zu\n", pos_a, pos_x); return false; }
    ts.words += (long)pos_x;
    return true;
}

int main() {
    const double inf = INFINITY, nan = NAN;
    Rng g{0x9e3779b97f4a7c15ull};
    // ---- the constants against their derivation (DESIGN §8 "Round 10")
    const double delta = NM_MF_ETA_S + 2.2e-8 + 0x1p-22 + 2e-15;
    if (!((2 * NM_MF_MAX_MD + 2) * delta <= EPS)) { bad++; printf("EPS_MAX %g < %d * %g\n", EPS, 2 * NM_MF_MAX_MD + 2, delta); }
    if (!(2 * EPS + 40 * 0x1p-24 + NM_MF_ETA_E + 0x1p-22 + 4 * 0x1p-24 <= KAPPA)) { bad++; printf("kappa %g too small\n", KAPPA); }
    if (!((double)NM_MF_DMIN >= 4 * EPS && (double)NM_MF_EMIN >= 4 * EPS)) { bad++; printf("DMIN / EMIN too small\n"); }

    // ---- (b) error bounds, every f32 in [-40, 0]
    {
        const uint32_t end = 0x42200000u + 1u;         // bits of 40.0f, inclusive
        unsigned nt = std::thread::hardware_concurrency();
        nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
        std::vector<double> me(nt), ms(nt);
        std::vector<long> oor(nt);
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; ++i) {
            const uint32_t lo = (uint32_t)((uint64_t)end * i / nt), hi = (uint32_t)((uint64_t)end * (i + 1) / nt);
            th.emplace_back(sweep, lo, hi, &me[i], &ms[i], &oor[i]);
        }
        for (auto& t : th) t.join();
        double max_e = 0., max_s = 0.;
        long o = 0;
        for (unsigned i = 0; i < nt; ++i) { if (!(me[i] <= max_e)) max_e = me[i]; if (!(ms[i] <= max_s)) max_s = ms[i]; o += oor[i]; }
        printf("(b) %u arguments: mf_exp max relative error %.3e (eta_e %.1e), mf_log1p(mf_exp) max absolute error %.3e (eta_s %.1e), %ld results outside (0, 1]\n",
               end, max_e, NM_MF_ETA_E, max_s, NM_MF_ETA_S, o);
        if (!(max_e <= NM_MF_ETA_E) || !(max_s <= NM_MF_ETA_S) || o) bad++;
    }
    // logaddexp_sl is merge_math_impl's total
    for (int i = 0; i < 1000000; ++i) {
        double a = (g.unif() - 0.5) * 100.0, b = i % 3 == 0 ? a : (i % 3 == 1 ? a + (g.unif() - 0.5) * 1e-3 : (g.unif() - 0.5) * 1600.0);
        if (d2u(logaddexp_sl(a, b)) != d2u(merge_math_impl(a, b, 0u, 0u, 0u).total)) { if (bad++ < 20) printf("logaddexp_sl(%a, %a) differs\n", a, b); }
    }
    for (double a : {0.0, -0.0, inf, -inf, nan, 1.0, 800.0}) for (double b : {0.0, -0.0, inf, -inf, nan, 1.0, -800.0}) {
        const double x = logaddexp_sl(a, b), y = merge_math_impl(a, b, 0u, 0u, 0u).total;
        if (d2u(x) != d2u(y) && !(x != x && y != y)) { if (bad++ < 20) printf("logaddexp_sl(%a, %a) differs\n", a, b); }
    }

    // ---- (a) soundness: the grid
    {
        const double M = 0x1p30;
        std::vector<double> sp = {0.0, -0.0, 1.0, -1.0, 1e-300, 5e-324, 0.5, -0.5, 3.5, -3.5, 36.0, 36.7, -36.7, 37.5, 40.0, -40.0, 52.0, 700.0, -700.0, 709.0, -709.8, 745.0, -745.2,
                                  1e6, -1e6, M, -M, M - 1.0, M + 1.0, -M - 1.0, std::nextafter(M, 0.0), std::nextafter(M, inf), M - 2 * EPS, M + 2 * EPS, 2 * M, 1e308, -1e308, inf, -inf, nan};
        std::vector<double> ds = {0.0, 5e-324, 0x1p-1022};
        for (int k = 52; k >= 10; --k) ds.push_back(std::ldexp(1.0, -k));                 // 1 ulp of 1.0 .. 2^-10
        for (double x : {(double)NM_MF_DMIN, 2 * EPS, 36.6, 36.7, 36.8, 39.99, 40.0, 40.01, 708.9, 709.0, 709.78, 709.79, 744.4, 745.0, 745.13, 745.14, 746.0, 9.0, 9.7, 10.4, 0.6931471805599453}) ds.push_back(x);
        auto words_for = [&](double a, double b, uint32_t is_main, std::vector<uint64_t>& ws) {
            ws = {0ull, ~0ull, 0x8000000000000000ull, 1ull, 0x00000000ffffffffull, 0x0000000100000000ull, 0xffffffff00000000ull, 0xffffffff00000001ull, 0x00000000ffffff01ull};
            const double p = exact_p(a, b, is_main);
            if (p >= 0.0 && p <= 1.0)
                for (double rel : {-2 * KAPPA, -KAPPA, -0.5 * KAPPA, 0.0, 0.5 * KAPPA, KAPPA, 2 * KAPPA}) for (int64_t off : {-1, 0, 1}) ws.push_back(word_at(p, rel, off) | 1ull);
        };
        std::vector<uint64_t> ws;
        for (uint32_t is_main : {0u, 1u}) {
            for (double a : sp) for (double b : sp) { words_for(a, b, is_main, ws); for (uint64_t w : ws) sound_all(a, b, is_main, w); }
            for (double a : sp) for (double d : ds) for (double sg : {1.0, -1.0}) {
                const double b = a + sg * d;
                words_for(a, b, is_main, ws); for (uint64_t w : ws) sound_all(a, b, is_main, w);
                const double a2 = std::nextafter(a, sg * inf);                               // +-1 ulp of the operand itself
                words_for(a2, a, is_main, ws); for (uint64_t w : ws) sound_all(a2, a, is_main, w);
            }
        }
    }
    // ---- (a) soundness: 1.2e7 random cases
    long und7 = 0, n7 = 0;
    for (int i = 0; i < 12000000; ++i) {
        const int kind = i % 8;
        const uint32_t is_main = (uint32_t)(g.next() & 1u);
        double a = (g.unif() - 0.5) * 40.0, b = (g.unif() - 0.5) * 40.0;
        uint64_t w = g.next();
        if (kind == 1) b = a + (g.unif() - 0.5) * std::ldexp(1.0, -(int)(g.next() % 44) - 8);
        if (kind == 2) { a = (g.next() & 1 ? 1.0 : -1.0) * 0x1p30 + (g.unif() - 0.5) * 8.0; b = a - (g.unif() - 0.5) * 60.0; }
        if (kind == 3) b = a;
        if (kind == 4) { const double c[6] = {36.7, -36.7, 709.0, -709.0, 745.0, -745.0}; b = a - c[g.next() % 6] + (g.unif() - 0.5) * 4.0; }
        if (kind == 5 || kind == 6) {                    // a word around the Bernoulli threshold; |a - b| where p is neither tiny nor 1
            b = a + (g.unif() - 0.5) * (kind == 5 ? 10.0 : 50.0);
            const double p = exact_p(a, b, is_main);
            if (p >= 0.0 && p < 1.0) w = word_at(p, (g.unif() - 0.5) * 4.0 * KAPPA, (int64_t)(g.next() % 3) - 1);
            if (g.next() % 16 == 0) w = (w & 0xffffffffull) | (g.next() & 1 ? 0xffffffff00000000ull : 0ull);     // w_hi 0 and 2^32 - 1
        }
        if (kind == 7) {                                 // the undecided share: |a - b| <= 5, uniform words, exact operands, not forced
            b = a + (g.unif() - 0.5) * 10.0;
            w |= 1ull;
            n7++;
            if (merge_filter_impl(a, b, is_main, (uint32_t)w, (uint32_t)(w >> 32)).flags == NM_MF_UNDECIDED) und7++;
        }
        const int pk = (int)(g.next() % 4);
        const double da = pk == 0 ? EPS : (pk == 1 ? -EPS : (g.unif() - 0.5) * 2 * EPS), db = pk == 0 ? -EPS : (pk == 1 ? EPS : (g.unif() - 0.5) * 2 * EPS);
        sound(a, b, is_main, w, da, db);
    }
    const double share = (double)und7 / (double)n7;
    printf("(a) %ld cases, %ld decided; undecided share on uniform words, |a - b| <= 5, not forced: %.3e (2 kappa = %.3e, bound 4 kappa = %.3e)\n", n_sound, n_decided, share, 2 * KAPPA, 4 * KAPPA);
    if (!(share <= 4 * KAPPA) || n_decided < n_sound / 10) { bad++; printf("the filter decides too little\n"); }
    // the forced exact path: a word with NM_MF_FORCE_BITS zero low bits is undecided whatever the operands
    for (int i = 0; i < 100000; ++i) {
        const uint64_t w = g.next() & ~((1ull << NM_MF_FORCE_BITS) - 1ull);
        if (merge_filter_impl((g.unif() - 0.5) * 10, (g.unif() - 0.5) * 10, (uint32_t)(i & 1), (uint32_t)w, (uint32_t)(w >> 32)).flags != NM_MF_UNDECIDED) { if (bad++ < 20) printf("forced word %016llx decided\n", (unsigned long long)w); }
    }

    // ---- (c) whole trees
    {
        TreeStats ts;
        long trees = 0;
        for (int i = 0; i < 120000; ++i) {
            const int law = i % 4, depth = 1 + (int)(g.next() % 10);
            if (law == 3 && depth > 7 && i % 16 != 3) continue;          // (all-equal weights replay every merge: the deep ones once in four)
            run_tree(g, depth, law, ts);
            trees++;
        }
        printf("(c) %ld trees, %ld merges, %ld replayed, %ld words consumed, max |L~ - L| %.3e (eps_max %.3e)\n", trees, ts.merges, ts.replays, ts.words, ts.max_err, EPS);
        if (trees < 100000 || ts.replays == 0) bad++;
    }
    printf("%ld mismatches\n", bad);
    return bad ? 1 : 0;
}
