// rank_score.hpp — the normal score of a rank (nm_transform_draws, include/nuts_amd.h): Phi^-1((r - 3/8) / (n + 1/4)) by Wichura's
// AS241 (PPND16), r = rank2 / 2 the 1-based average rank.  ONE function for the score kernel (rank_transform.hip) and for its host twin
// nm_rank_normal_score: the same operation sequence on both sides (the engine = host twin pattern of §23), every step one binary64 operation
// (the build's -ffp-contract=off), the logarithm dev_math.hpp's dlog.  The argument stays in integers as long as it can, which makes the
// score exactly antisymmetric: score(n, 2n + 2 - rank2) == -score(n, rank2) bit for bit, and score(n, n + 1) == +0.0.
// On the device the kernel calls nm::dm_init_lds() first (dlog's tables live in LDS there).
#pragma once
#include "dev_math.hpp"

namespace nm {
// degree-7 Horner evaluation from the top coefficient; the coefficients come low order first, as AS241 lists them
NM_HD double rank_poly7(double r, double c0, double c1, double c2, double c3, double c4, double c5, double c6, double c7) {
    double p = c7;
    p = p * r + c6;
    p = p * r + c5;
    p = p * r + c4;
    p = p * r + c3;
    p = p * r + c2;
    p = p * r + c1;
    p = p * r + c0;
    return p;
}

// n in 1 .. 2^31 - 1, rank2 in 2 .. 2n (the callers check): A <= 8n - 3 and 2B = 16n + 4 are exact in a double
NM_HD double rank_normal_score(uint64_t n, uint64_t rank2) {
    const uint64_t A = 4 * rank2 - 3, B = 8 * n + 2;
    const double q = (double)(int64_t)(2 * A - B) / (double)(2 * B);
    const double aq = q < 0.0 ? -q : q;
    if (aq <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = rank_poly7(r, 3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
                                      4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3);
        const double den = rank_poly7(r, 1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
                                      2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3);
        return q * num / den;
    }
    const uint64_t m = A < B - A ? A : B - A;
    const double t = (double)m / (double)B;
    double r = __builtin_sqrt(-dlog(t));
    double w;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = rank_poly7(r, 1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
                                      1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4);
        const double den = rank_poly7(r, 1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
                                      1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9);
        w = num / den;
    } else {
        r -= 5.0;
        const double num = rank_poly7(r, 6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
                                      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7);
        const double den = rank_poly7(r, 1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                                      7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15);
        w = num / den;
    }
    return q < 0.0 ? -w : w;
}
}  // namespace nm
