// fpldpc_float_state.hpp -- the floating-point decoder's per-decoder state (fpldpc_float.hip builds and
// uses it; fpldpc_float_describe.cpp reads it for the test-only fpldpc_testing_float_describe).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace fpldpc {

struct FloatState {
    int device = -1;
    int grid = 0;             // resident workgroups
    size_t lds = 0;
    const void *fn = nullptr;    // the kernel (a __global__ void (FArgs) of fpldpc_float.hip)
    int32_t *d_cvar = nullptr;   // [dc_max][m] var of slot k of check c (-1 pad)
    uint8_t *d_cdeg = nullptr;   // [m]
    int32_t *d_vedge = nullptr;  // [dv_max][n] edge index slot*m + c of the k-th check of v
    uint8_t *d_vdeg = nullptr;   // [n]
    double *d_msg = nullptr;     // [grid][planes][dc_max * m]: edge messages (+ forward chain, generic kernel)
    int planes = 2;
    int *d_counter = nullptr;
    ~FloatState() {
        (void)hipFree(d_cvar);
        (void)hipFree(d_cdeg);
        (void)hipFree(d_vedge);
        (void)hipFree(d_vdeg);
        (void)hipFree(d_msg);
        (void)hipFree(d_counter);
    }
};

}  // namespace fpldpc
