// fpldpc_layered_host.hpp -- host code the layered units share (fpldpc_layered.hip, fpldpc_layered_minsum.hip,
// fpldpc_minsum.hip, fpldpc_minsum_global.hip, fpldpc_flood_sat.hip, fpldpc_flood_sat_global.hip): the steps of a kernel choice (degree bucket, residency probe,
// index-table placement, grid) and the launch.  Templates over the kernel's function pointer: the kernels are
// templates in each unit's anonymous namespace.  `who` is the decoder's name in the error texts ("layered",
// "layered min-sum", "flooding min-sum", "saturated flooding").  Included by those translation units only, after
// fpldpc_layered_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "fpldpc_layered_device.hpp"

namespace fpldpc {
namespace {

// f(DC, EXACT) as compile-time constants for a choice's (dc, exact): the exact degree 47, else one of the
// buckets; null for anything else.
template <typename F>
auto lay_for_dc(int dc, bool exact, F f) -> decltype(f(std::integral_constant<int, 8>{}, std::false_type{})) {
    if (exact) return f(std::integral_constant<int, kExactDc>{}, std::true_type{});
    switch (dc) {
        case 8: return f(std::integral_constant<int, 8>{}, std::false_type{});
        case 16: return f(std::integral_constant<int, 16>{}, std::false_type{});
        case 32: return f(std::integral_constant<int, 32>{}, std::false_type{});
        case 48: return f(std::integral_constant<int, 48>{}, std::false_type{});
        case 64: return f(std::integral_constant<int, 64>{}, std::false_type{});
    }
    return nullptr;
}

// The part of a choice that the code alone decides: check degrees 2..64, the kernel's DC and addressing.
inline int lay_choice_of_code(const fpldpc_code &code, int mode, const char *who, LayeredChoice *lc) {
    for (int r = 0; r < code.m; r++)
        if (code.cdeg[r] < 2) return fail(FPLDPC_ERR_UNSUPPORTED, "check of degree < 2 (reference behaviour undefined)");
    int dc = 0;
    for (int d : {8, 16, 32, 48, 64})
        if (!dc && code.dc_max <= d) dc = d;
    if (!dc) return fail(FPLDPC_ERR_UNSUPPORTED, std::string(who) + " decoder: check degree above 64");
    lc->mode = mode;
    lc->exact = code.regular_checks && code.dc_max == kExactDc;
    lc->dc = lc->exact ? kExactDc : dc;
    lc->computed = code.array_forward && code.array_p > 0;
    return FPLDPC_OK;
}

// Resident workgroups per CU of `fn` with `lds` bytes of dynamic LDS (0 once an error is in `e`, which sticks).
template <typename Fn>
struct LayResidency {
    Fn fn;
    int threads;
    hipError_t e = hipSuccess;
    int operator()(size_t lds) {
        int per_cu = 0;
        if (e == hipSuccess && lds > 64 * 1024) e = raise_dynamic_lds((const void *)fn, lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds);
        return e == hipSuccess ? per_cu : 0;
    }
};

// The index table (tab_bytes; 0: computed addressing) joins the `base` bytes in LDS only where it fits and
// costs no resident workgroup; the environment variable `env` = global / lds places a table that fits regardless.
template <typename Fn>
bool lay_table_in_lds(const char *env, size_t base, size_t tab_bytes, LayResidency<Fn> &resident) {
    if (!tab_bytes || base + tab_bytes > kLdsMax) return false;
    const char *table = getenv(env);
    if (table && (!strcmp(table, "lds") || !strcmp(table, "global"))) return !strcmp(table, "lds");
    return resident(base + tab_bytes) == resident(base);
}

// Occupancy (per_cu and the probe's error) to the persistent grid: per_cu workgroups on every CU of `device`.
inline int lay_grid(int per_cu, hipError_t probe, int device, const char *who, int *grid) {
    if (probe != hipSuccess) return fail_hip(probe, (std::string(who) + " kernel occupancy").c_str());
    if (per_cu < 1) return fail(FPLDPC_ERR_UNSUPPORTED, std::string(who) + " kernel cannot be resident (occupancy 0)");
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    *grid = per_cu * prop.multiProcessorCount;
    return FPLDPC_OK;
}

inline const char *lay_addr_name(const LayeredChoice &lc) { return lc.computed ? "computed" : lc.table_lds ? "table" : "gtable"; }

// The rest of the choice of a decoder whose state is all in LDS (the two min-sum decoders), from `base`
// bytes of it: table placement, LDS bytes, grid and the name `kernel`<...>.
template <typename Fn>
int lay_choose_lds(Fn fn, const fpldpc_code &code, size_t base, const char *env, int device, const char *who,
                   const char *kernel, LayeredChoice *lc) {
    const size_t tab_bytes = lc->computed ? 0 : (size_t)code.dc_max * code.m * sizeof(uint16_t);
    LayResidency<Fn> resident{fn, lc->threads};
    lc->lds_state = true;
    lc->table_lds = lay_table_in_lds(env, base, tab_bytes, resident);
    lc->lds_bytes = base + (lc->table_lds ? tab_bytes : 0);
    const int per_cu = resident(lc->lds_bytes);
    if (int st = lay_grid(per_cu, resident.e, device, who, &lc->grid)) return st;
    snprintf(lc->name, sizeof lc->name, "%s<DC=%d,addr=%s,deg=%s>", kernel, lc->dc, lay_addr_name(*lc),
             lc->exact ? "exact" : "table");
    return FPLDPC_OK;
}

// Launches fn(kargs) as `lc` chose it over the frames of `a` (the LayeredArgs inside kargs).
template <typename Fn, typename KArgs>
int lay_launch(Fn fn, const LayeredChoice &lc, const LayeredArgs &a, const KArgs &kargs, void *stream, const char *who) {
    if (a.batch <= 0) return FPLDPC_OK;
    if (!fn) return fail(FPLDPC_ERR_ARG, std::string(who) + " decoder has no kernel");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fn, dim3(std::min(lc.grid, a.batch)), dim3(lc.threads), lc.lds_bytes, s, kargs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        // a launch that fails leaves the counter block for the next call to find non-zero: re-zero it
        (void)hipMemsetAsync(a.counters, 0, kLayeredCounterInts * sizeof(int32_t), s);
        return fail_hip(e, (std::string(who) + " kernel launch").c_str());
    }
    return FPLDPC_OK;
}

}  // namespace
}  // namespace fpldpc
