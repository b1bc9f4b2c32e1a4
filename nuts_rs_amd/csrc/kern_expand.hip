// kern_expand.hip — the expansion pass (nuts_expand.hpp) for the built-in densities: nm_expand_kernel<Density> for every functor of
// nuts_kernels.hpp that defines expanded_dim / expand_element (today: the non-centred 8 schools -> (mu, tau, theta[8])).  The others expand to
// the position itself; the engine serves them with a device-to-device copy and no kernel exists for them.
#include "nuts_expand.hpp"

namespace nm {

template <class Dens>
static uint64_t expanded_dim_t(uint64_t dim, const double* h_params, uint64_t n_params, int* has_kernel) {
    *has_kernel = has_expand<Dens>::value ? 1 : 0;
    if constexpr (has_expand<Dens>::value) return Dens::expanded_dim(dim, h_params, n_params);
    else return dim;
}

uint64_t builtin_expanded_dim(uint64_t logp_kind, uint64_t dim, const double* h_params, uint64_t n_params, int* has_kernel) {
    switch (logp_kind) {
    case NM_LOGP_IID_NORMAL: return expanded_dim_t<IidNormal>(dim, h_params, n_params, has_kernel);
    case NM_LOGP_DIAG_NORMAL: return expanded_dim_t<DiagNormal>(dim, h_params, n_params, has_kernel);
    case NM_LOGP_FUNNEL: return expanded_dim_t<Funnel>(dim, h_params, n_params, has_kernel);
    case NM_LOGP_EIGHT_SCHOOLS: return expanded_dim_t<EightSchools>(dim, h_params, n_params, has_kernel);
    case NM_LOGP_MVN_PREC: return expanded_dim_t<MvnPrec>(dim, h_params, n_params, has_kernel);
    }
    *has_kernel = 0;          // NM_LOGP_HOST_CALLBACK: the host function has the reference's default, the position itself
    return dim;
}

hipError_t launch_expand(uint64_t logp_kind, const double* d_params, uint64_t dim, uint64_t edim, uint64_t n_rows, const double* d_positions,
                         double* d_expanded, unsigned grid_cap, hipStream_t stream) {
    switch (logp_kind) {      // (a density without an expansion answers hipErrorInvalidValue: a missing kernel is an error, never a silent copy here)
    case NM_LOGP_IID_NORMAL: return launch_expand_t<IidNormal>(d_params, dim, edim, n_rows, d_positions, d_expanded, grid_cap, stream);
    case NM_LOGP_DIAG_NORMAL: return launch_expand_t<DiagNormal>(d_params, dim, edim, n_rows, d_positions, d_expanded, grid_cap, stream);
    case NM_LOGP_FUNNEL: return launch_expand_t<Funnel>(d_params, dim, edim, n_rows, d_positions, d_expanded, grid_cap, stream);
    case NM_LOGP_EIGHT_SCHOOLS: return launch_expand_t<EightSchools>(d_params, dim, edim, n_rows, d_positions, d_expanded, grid_cap, stream);
    case NM_LOGP_MVN_PREC: return launch_expand_t<MvnPrec>(d_params, dim, edim, n_rows, d_positions, d_expanded, grid_cap, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace nm
