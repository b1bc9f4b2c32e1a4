// The fma chains of nm_pooled_scatter's definition (include/nuts_amd.h) on the host, for tests/scatter_ref.py: numpy has no fused
// multiply-add.  Compiled with -ffp-contract=off: the only fused operations are the std::fma calls written here.
#include <cmath>
#include <cstdint>
#include <vector>

// S[dim][dim] of the kept rows (keep: one byte per row, or null = every row), slabs of slab_rows rows, n_slabs of them
extern "C" void scatter_ref(uint64_t n_rows, uint64_t dim, const double* x, const double* c, const uint8_t* keep, uint64_t slab_rows,
                            uint64_t n_slabs, double* S) {
    std::vector<double> y(dim), acc(dim * dim);
    for (uint64_t e = 0; e < dim * dim; ++e) S[e] = 0.0;
    for (uint64_t s = 0; s < n_slabs; ++s) {
        for (uint64_t e = 0; e < dim * dim; ++e) acc[e] = 0.0;
        const uint64_t r0 = s * slab_rows, r1 = (s + 1) * slab_rows < n_rows ? (s + 1) * slab_rows : n_rows;
        for (uint64_t r = r0; r < r1; ++r) {
            if (keep && !keep[r]) continue;
            for (uint64_t d = 0; d < dim; ++d) y[d] = x[r * dim + d] - c[d];
            for (uint64_t i = 0; i < dim; ++i)
                for (uint64_t j = 0; j < dim; ++j) acc[i * dim + j] = std::fma(y[i], y[j], acc[i * dim + j]);
        }
        for (uint64_t e = 0; e < dim * dim; ++e) S[e] = S[e] + acc[e];
    }
}
