// A USER density with an expansion (include/nuts_amd.h, "User densities": expanded_dim / expand_element): the diagonal normal of
// my_diag_normal.hpp, read by its user as (exp(x_0), ..., exp(x_{dim-1}), x_0 * x_{dim-1}) — dim + 1 numbers per draw.
//   expanded_dim   the length of the expanded vector, callable on the host
//   expand_element element j of the expansion of the row x[0 .. dim): a function of (params, x, j) alone.  Lanes of a wavefront work on
//                  different rows here, so the special functions are the per-lane, always-inlined ones (nm::xexp), never the
//                  wave-uniform nm::uexp of `eval`.
#pragma once
#include "my_diag_normal.hpp"

struct MyExpandingNormal : MyDiagNormal {
    static NM_HD uint64_t expanded_dim(uint64_t dim, const double*, uint64_t) { return dim + 1; }
    static NM_DEV double expand_element(const double*, int dim, const double* x, int j) {
        if (j < dim) return nm::xexp(x[j]);
        return x[0] * x[dim - 1];
    }
};
