// merge_math_main_check.hip — HOST program (compiled with hipcc, runs on the CPU): the main-tree merge with one exp (csrc/dev_math.hpp
// merge_math_main) against merge_math_impl(.., is_main = 1, ..), `total` and `flags` bit for bit, over the special operands of
// merge_math_check.hip and 1e6 random pairs.  Exit code 0 = identical everywhere.
#include "../../nuts_rs_amd/csrc/dev_math.hpp"
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>
using namespace nm;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double unif() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
int main() {
    long bad = 0, n = 0;
    const double inf = INFINITY, nan = NAN;
    // +-0, +-inf, NaN, equal operands, sub-normal differences, |diff| around 709 and 745 (where exp overflows / underflows)
    std::vector<double> sp = {0.0, -0.0, 1.0, -1.0, 1e-300, -1e-300, 5e-324, -5e-324, 0x1p-1074, 0x1p-1022, 0x1.fffffffffffffp-1023, 700.0, -700.0, 745.0, -745.2, -746.0,
                              745.13, 745.14, 708.0, 709.7, 709.8, 710.0, -709.7, -709.8, 1e308, -1e308, inf, -inf, nan, 0.5, -0.5, 36.0, -36.0, 37.5, -37.5, 1e-17, -1e-17,
                              0.6931471805599453, -0.6931471805599453, 3.5, -3.5, 52.0, -53.0, 1075.0, -1075.0};
    auto check = [&](double a, double b, uint64_t w) {
        const MergeOut r = merge_math_impl(a, b, 1u, (uint32_t)w, (uint32_t)(w >> 32));
        const MergeOut o = merge_math_main(a, b, (uint32_t)w, (uint32_t)(w >> 32));
        n++;
        if (d2u(r.total) != d2u(o.total) || r.flags != o.flags) {
            if (bad++ < 20) printf("merge_math_main(%a, %a, w %016llx): total %a flags %u, merge_math_impl %a flags %u\n", a, b, (unsigned long long)w, o.total, o.flags, r.total, r.flags);
        }
    };
    for (double a : sp) for (double b : sp) for (uint64_t w : {0ull, ~0ull, 0x8000000000000000ull, 1ull}) check(a, b, w);
    for (double a : sp) for (double d : {5e-324, 1e-310, 0x1p-1022, 708.9, 709.0, 709.78, 709.79, 744.4, 745.0, 745.13, 745.14, 746.0}) for (uint64_t w : {0ull, ~0ull}) {
        check(a, a - d, w); check(a, a + d, w); check(a - d, a, w); check(a + d, a, w);
    }
    for (int i = 0; i < 1000000; ++i) {
        const int kind = i % 6;
        double a = (unif() - 0.5) * 40.0, b = (unif() - 0.5) * 40.0;
        if (kind == 1) b = a + (unif() - 0.5) * 1e-3;
        if (kind == 2) { a *= 40.0; b *= 40.0; }
        if (kind == 3) b = a;
        if (kind == 4) b = a - unif() * 800.0;
        uint64_t w = next();
        if (kind == 5) {                     // a word right at the Bernoulli threshold
            const double p = exp_sl(b - a);
            if (p >= 0.0 && p < 1.0) w = (uint64_t)(p * 18446744073709551616.0) + (uint64_t)((i >> 4) % 3) - 1;
        }
        check(a, b, w);
    }
    printf("%ld comparisons, %ld mismatches\n", n, bad);
    return bad ? 1 : 0;
}
