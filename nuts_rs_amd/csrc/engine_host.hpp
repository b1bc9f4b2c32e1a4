// engine_host.hpp — what the C entry points outside nuts_engine.hip (unit_batch.hip) share with the engine: the one error string
// behind nm_last_error, the device and density checks, the stream-ordered copy.  All defined in nuts_engine.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include "../../include/nuts_amd.h"
namespace nm { namespace host {
nm_status fail(nm_status st, const char* fmt, ...);      // sets the calling thread's nm_last_error, returns st
nm_status ensure_device(int64_t device);                 // a HIP device exists (and `device` >= 0 is made current)
nm_status check_logp(const nm_logp_spec* l);
int pick_dpl(uint64_t dim, uint64_t requested);          // doubles per lane of a one-wavefront tiling for `dim` (0: none)
hipError_t copy_on(hipStream_t s, void* dst, const void* src, size_t n, hipMemcpyKind kind);      // enqueue on `s`, wait for `s` (stream discipline)
extern const double* const zig_tables;                   // rand_distr's ZIG_NORM_X then ZIG_NORM_F: 2 x 257 doubles
} }  // namespace nm::host
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return nm::host::fail(NM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
