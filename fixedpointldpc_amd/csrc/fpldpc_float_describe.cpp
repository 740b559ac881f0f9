// fpldpc_float_describe.cpp -- fpldpc_testing_float_describe (include/fpldpc_testing.h): which kernel
// the floating-point decoder of a decoder launches, for the tests that must know which form they ran.
//
// A translation unit of its own, outside the kernel build id (fixedpointldpc_amd/_build.py HASHED_TUS):
// the entry point changes nothing that runs on the GPU or how it is chosen, so the committed counters
// stay those of the shipped kernels.  It therefore reads, and does not repeat, the choice that
// float_setup (fpldpc_float.hip) made: the kernel's name as the HIP runtime knows the function pointer
// the decoder launches.
#include <cstdio>
#include <cstring>
#include <string>

#include <hip/hip_runtime_api.h>

#include "fpldpc_float_state.hpp"
#include "fpldpc_host.hpp"
#include "fpldpc_testing.h"

using namespace fpldpc;

namespace {

// "bp_float_reg<DC=47,regular,array>" from the kernel's mangled name (..bp_float_regILi47ELb1ELb1EE..:
// DC, REGULAR, ARRAY of fpldpc_float.hip), "bp_float_kernel" for the generic kernel; "" if neither
std::string float_kernel_form(const char *mangled) {
    const std::string s = mangled ? mangled : "";
    if (s.find("bp_float_kernel") != std::string::npos) return "bp_float_kernel";
    const size_t at = s.find("bp_float_regILi");
    int dc = 0, regular = 0, array = 0;
    if (at == std::string::npos || sscanf(s.c_str() + at, "bp_float_regILi%dELb%1dELb%1dE", &dc, &regular, &array) != 3)
        return "";
    return "bp_float_reg<DC=" + std::to_string(dc) + (regular ? ",regular" : ",predicated") + (array ? ",array>" : ",table>");
}

}  // namespace

extern "C" int fpldpc_testing_float_describe(void *decoder, char *buf, int32_t len) {
    fpldpc_decoder *dec = static_cast<fpldpc_decoder *>(decoder);
    if (!dec || !buf || len <= 0) return fail(FPLDPC_ERR_ARG, "null decoder or buffer");
    if (!dec->fl) {
        // the tables and the kernel choice are built by the first decode: one all-zero frame, no outputs
        DeviceGuard g(dec->device);
        if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
        double *llr = nullptr;
        const size_t bytes = sizeof(double) * (size_t)dec->code.n;
        hipError_t e = hipMalloc((void **)&llr, bytes);
        if (e == hipSuccess) e = hipMemset(llr, 0, bytes);
        int st = e == hipSuccess ? fpldpc_decode_float(dec, llr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)
                                 : fail_hip((int)e, "float describe: frame allocation");
        if (e == hipSuccess && st == FPLDPC_OK) {
            e = hipDeviceSynchronize();
            if (e != hipSuccess) st = fail_hip((int)e, "float describe: first decode");
        }
        (void)hipFree(llr);
        if (st != FPLDPC_OK) return st;
    }
    const FloatState *s = dec->fl;
    std::string form = float_kernel_form(hipKernelNameRefByPtr(s->fn, nullptr));
    if (form.empty()) {  // the same name by way of the function handle
        hipFunction_t f = nullptr;
        if (hipGetFuncBySymbol(&f, s->fn) == hipSuccess && f) form = float_kernel_form(hipKernelNameRef(f));
    }
    if (form.empty()) return fail(FPLDPC_ERR_HIP, "float describe: the runtime does not name the float kernel");
    snprintf(buf, (size_t)len, "%s grid=%d planes=%d", form.c_str(), s->grid, s->planes);
    return FPLDPC_OK;
}
