// fpldpc_kernels.hip -- gfx950 (CDNA4) flooding decoder for the reference's fixed-point LDPC path: the
// host side.  The table of kernel variants (kVariants), the choice among them (choose_kernel) and the
// launches (launch_decode: a packed kernel and its fallback chain; launch_decode_frame: the stateful
// single-frame decode).  The kernels are in the fpldpc_flood_*.hpp headers (fpldpc_flood_device.hpp
// has the design); this unit instantiates all of them but A's and the degree-sorted W's, which
// fpldpc_kernels_a1.hip and fpldpc_kernels_w1.hip compile with options of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "fpldpc_internal.hpp"
#include "fpldpc_testing.h"

// (in this order, not the alphabet's: the order of the kernels' definitions is the order of their
// sections in the object, which the kernel build id covers)
#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_int32.hpp"
#include "fpldpc_flood_packed.hpp"
#include "fpldpc_flood_checks_array.hpp"
#include "fpldpc_flood_checks_table.hpp"
#include "fpldpc_flood_pk.hpp"
#include "fpldpc_flood_lds16.hpp"

namespace fpldpc {

// the A and W kernels' host stubs (fpldpc_kernels_a1.hip, fpldpc_kernels_w1.hip, compiled separately)
const void *array47_pair_kernel();
const void *array47_pair_outguard_kernel();
const void *table8_pair_kernel();

namespace {

typedef void (*KernelFn)(KArgs);

struct VariantInfo {
    Variant v;
    KernelFn fn;
    int dc;       // kernel DC
    int max_m;    // 0 = any
    bool regular; // requires every check degree == dc
    bool gmem;
    const char *name;
    int array_p = 0;  // > 0: forward array code with this p only (computed addressing)
    bool low_mask = false;  // width_mask must be 2^w - 1 (bit-field extract)
    Variant fallback = Variant::kNone;  // int32 kernel re-decoding frames the packed kernel rejects
    int nt = kNT;           // threads per workgroup
    bool lds_state = false; // c2v state in LDS (int16 [dc][m])
    int dmin = 2;           // smallest check degree the variant handles
    int tab_words = 0;      // LDS table words per check after the control words (array LDS offsets)
    int lo_passes = 0;      // > 0: checks listed by ascending degree, the first lo_passes * nt of degree dmin
    int chain_guard = 0;    // > 0: range guard from two chain values, needs chain_guard * C <= (cmax + 1) / 8
    int stat_words = 0;     // > 0: flood_pk's stationary exit, this many scratch words per workgroup
};

size_t variant_lds(const VariantInfo &x, const fpldpc_code &c) {
    size_t b = (size_t)(4 * c.n + kMiscInts) * sizeof(int);
    if (x.lds_state) b += (size_t)c.m * x.dc * sizeof(int16_t);
    b += (size_t)c.m * x.tab_words * sizeof(uint32_t);
    // flood_pk: the info masks staged in LDS.  The int32 kernels (no fallback: flood_array, flood_reg,
    // flood_gmem) use nothing past the control words and have no static LDS, so they are not charged for
    // the masks: their longest code is the one choose_kernel's length test admits, (4 n + 20) * 4 <= 160 KiB,
    // n = 10,235; the int16 kernels' envelopes stay as they were.
    if (x.fallback != Variant::kNone) b += 2 * (size_t)((c.n + 31) / 32) * sizeof(uint32_t);
    return b;
}

const VariantInfo kVariants[] = {
    // A: the chain range guard (G = 24 C) while it is a small share of cmax, else the same kernel with
    // the per-output guard (chain_guard_ok)
    {Variant::kArray47x2, reinterpret_cast<KernelFn>(const_cast<void *>(array47_pair_kernel())), 47, kNT, true, false,
     "flood_array2<P=47,W=3>", 47, true, Variant::kArray47, kNT, false, 2, 0, 0, (47 - 1) / 2 + 1, ArrayChecks<47>::kStatWords},
    {Variant::kArray47x2og, reinterpret_cast<KernelFn>(const_cast<void *>(array47_pair_outguard_kernel())), 47, kNT, true, false,
     "flood_array2<P=47,W=3>", 47, true, Variant::kArray47, kNT, false, 2, 0, 0, 0, ArrayChecks<47>::kStatWords},
    // p = 47 array codes with more than 256 checks, in one 768-thread workgroup at 3 waves / SIMD; the
    // first entry that fits the code is taken.  int16 range misses go to the LDS-state kernel and from
    // there to the global one.
    //   mix (R: 1128 checks; up to 1152): 2 checks per lane up to check 1024, the rest two lanes per
    //     check -- 4.5 check-units on every SIMD per step (+8.6 % over the next entry,
    //     profiles/r3/ab/r_mix.txt)
    //   CPL=2,ldsoffs (up to 1536 checks): 2 checks per lane, SIMD loads 5 / 5 / 4 / 4; the slot offsets
    //     in an LDS table (143 KB of LDS with R's), so no offset walking
    //   CPL=2: the same with the offsets walked per step
    {Variant::kArray47x2mix, flood_pk<MixChecks<47>, 1, 768>, 47, 768 + 256 + 128, true, false,
     "flood_array2<P=47,CPL=2,ldsoffs,mix>", 47, true, Variant::kLds16_47, 768, false, 2, MixChecks<47>::kTabWords},
    {Variant::kArray47x2c2t, flood_pk<ArrayChecks<47, 2, 768, true, true>, 1, 768>, 47, 2 * 768, true, false,
     "flood_array2<P=47,CPL=2,ldsoffs>", 47, true, Variant::kLds16_47, 768, false, 2, ArrayChecks<47, 2, 768, true, true>::kTabWords},
    {Variant::kArray47x2c2, flood_pk<ArrayChecks<47, 2, 768>, 1, 768>, 47, 2 * 768, true, false,
     "flood_array2<P=47,CPL=2>", 47, true, Variant::kLds16_47, 768},
    {Variant::kArray47, flood_array<47>, 47, kNT, true, false, "flood_array<P=47>", 47, true},
    // degrees 7..8 with at least 768 checks of degree 7 (W: 810 of 972): passes 0-2 fold 7 slots
    {Variant::kTab8x4lo3, reinterpret_cast<KernelFn>(const_cast<void *>(table8_pair_kernel())), 8, 4 * kNT, false, false,
     "flood_tab2<DC=8,CPL=4,lo=3>", 0, true, Variant::kReg8x4, kNT, false, 7, 0, 3},
    {Variant::kTab8x4p, flood_pk<TableChecks<8, 4, 7>, 4>, 8, 4 * kNT, false, false, "flood_tab2<DC=8,CPL=4>", 0, true,
     Variant::kReg8x4, kNT, false, 7},
    {Variant::kLds16_47, flood_lds16<47>, 47, 2 * kNT16, true, false, "flood_lds16<P=47>", 47, true, Variant::kGmem48,
     kNT16, true},
    {Variant::kReg47x1Regular, flood_reg<47, 1, true>, 47, kNT, true, false, "flood_reg<DC=47,CPL=1,regular>"},
    {Variant::kReg8x1, flood_reg<8, 1, false>, 8, kNT, false, false, "flood_reg<DC=8,CPL=1>"},
    {Variant::kReg8x4, flood_reg<8, 4, false>, 8, 4 * kNT, false, false, "flood_reg<DC=8,CPL=4>"},
    {Variant::kReg16x2, flood_reg<16, 2, false>, 16, 2 * kNT, false, false, "flood_reg<DC=16,CPL=2>"},
    {Variant::kGmem8, flood_gmem<8>, 8, 0, false, true, "flood_gmem<DC=8>"},
    {Variant::kGmem16, flood_gmem<16>, 16, 0, false, true, "flood_gmem<DC=16>"},
    {Variant::kGmem32, flood_gmem<32>, 32, 0, false, true, "flood_gmem<DC=32>"},
    {Variant::kGmem48, flood_gmem<48>, 48, 0, false, true, "flood_gmem<DC=48>"},
    {Variant::kGmem64, flood_gmem<64>, 64, 0, false, true, "flood_gmem<DC=64>"},
};

const VariantInfo *find_variant(Variant v) {
    for (const auto &x : kVariants)
        if (x.v == v) return &x;
    return nullptr;
}

}  // namespace

int fail_hip(int hip_status, const char *what) {
    return fail(FPLDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)hip_status));
}

int kernel_dc(Variant v) {
    const VariantInfo *vi = find_variant(v);
    return vi ? vi->dc : 0;
}

// int16 range of the packed kernels: with |LLR| <= kLlrMax and every c2v magnitude <= cm, |post| <=
// kLlrMax + dv*cm and |v2c| <= kLlrMax + (dv+1)*cm; a box-plus chain value is at most its last v2c
// input + C (bp_mag <= min + C: the WIDTH_MASK wrap can make part1 exceed part2), so every chain value
// stays below 2^15 -- magnitudes keep bit 15 clear and a + b never carries out of a 16-bit half -- when
// kLlrMax + (dv+1)*cm + max(64, C) <= 32767.  Returns the largest such cm = 2^b - 1, or 0 when not even
// cm = 1 fits (C = 5/8 * 2^FRAC_WIDTH, ArrayLDPCMacro.h:175: FRAC_WIDTH >= 16 on any code).
uint32_t packed_cmax(const fpldpc_code &code, int C) {
    const uint64_t margin = (uint64_t)std::max(64, C);
    auto fits = [&](uint64_t cm) { return (uint64_t)kLlrMax + (uint64_t)(code.dv_max + 1) * cm + margin <= 32767; };
    if (!fits(1)) return 0;
    uint32_t cm = 1;
    while (fits(2 * (uint64_t)cm + 1)) cm = 2 * cm + 1;
    return cm;
}

// The chain range guard (ArrayChecks::kChainGuard) flags a frame when max(F_{L-1}, B_{L+1}) + G reaches
// cmax + 1, G = (L+1) C: needlessly only when that maximum lies within G of the threshold.  It is used
// while G is at most an eighth of the range (C = 10: 240 of 4096); beyond that the per-output guard.
bool chain_guard_ok(int slots, int C, uint32_t cmax) {
    return (uint64_t)slots * (uint64_t)C <= ((uint64_t)cmax + 1) / 8;
}

// flood_lds16 is exact while |v2c| < 2^14 (checked per step): its chain values and c2v are then at
// most 2^14 - 1 + C, which its u16 minima and int16 c2v state hold while C <= 2^14 (FRAC_WIDTH <= 14).
constexpr int kLds16MaxC = 1 << 14;

int choose_kernel(const fpldpc_code &code, int device, int mask, int C, KernelChoice *out) {
    const bool low_mask = mask >= 3 && (mask & (mask + 1)) == 0;
    const uint32_t cmax = packed_cmax(code, C);
    // an int16 kernel, or a chain that hands frames down to one, is exact at this C
    auto int16_ok = [&](const VariantInfo &x) {
        for (const VariantInfo *y = &x; y; y = y->fallback == Variant::kNone ? nullptr : find_variant(y->fallback))
            if (y->lds_state && C > kLds16MaxC) return false;
        return x.fallback == Variant::kNone || x.lds_state || cmax > 0;
    };
    // the variant and every kernel of its fallback chain fit the LDS (setup_fallback makes each of them
    // resident: p = 47 with 1363..1504 checks fits the walked CPL=2 kernel but not its LDS-state fallback)
    auto lds_ok = [&](const VariantInfo &x) {
        for (const VariantInfo *y = &x; y; y = y->fallback == Variant::kNone ? nullptr : find_variant(y->fallback))
            if (variant_lds(*y, code) > 160 * 1024) return false;
        return true;
    };
    for (int r = 0; r < code.m; r++)
        if (code.cdeg[r] < 2) return fail(FPLDPC_ERR_UNSUPPORTED, "check of degree < 2 (reference behaviour undefined)");
    if (code.dc_max > 64) return fail(FPLDPC_ERR_UNSUPPORTED, "check degree above 64");
    if ((size_t)(4 * code.n + kMiscInts) * sizeof(int) > 160 * 1024)
        return fail(FPLDPC_ERR_UNSUPPORTED, "code length too large for LDS-resident posteriors");
    // The reference iterates its checks in block order and folds each in clist order; the kernel
    // folds in clist order per check, so only the degree envelope matters for the choice.
    int actual_dc = 0;
    for (int r = 0; r < code.m; r++) actual_dc = std::max(actual_dc, (int)code.cdeg[r]);
    bool regular = true;
    int min_dc = actual_dc;
    for (int r = 0; r < code.m; r++) {
        regular &= code.cdeg[r] == actual_dc;
        min_dc = std::min(min_dc, (int)code.cdeg[r]);
    }
    int n_min_dc = 0;  // checks of the smallest degree (listed first when a variant sorts them)
    for (int r = 0; r < code.m; r++) n_min_dc += code.cdeg[r] == min_dc;
    const VariantInfo *pick = nullptr;
    // FPLDPC_KERNEL=<name prefix> forces a variant (A/B measurements); it must still fit the code
    const char *force = getenv("FPLDPC_KERNEL");
    for (const auto &x : kVariants) {
        if (force && *force && strncmp(x.name, force, strlen(force)) != 0) continue;
        if (x.gmem) continue;
        if (x.array_p && !(code.array_p == x.array_p && code.array_forward)) continue;
        if (x.low_mask && !low_mask) continue;
        if (x.fallback != Variant::kNone && mask > 0xffff) continue;  // packed halves: mask within 16 bits
        if (!int16_ok(x)) continue;
        if (!lds_ok(x)) continue;
        if (min_dc < x.dmin) continue;
        if (x.regular ? !(regular && actual_dc == x.dc) : actual_dc > x.dc) continue;
        if (code.m > x.max_m) continue;
        if (x.lo_passes && !(min_dc == x.dmin && n_min_dc >= x.lo_passes * x.nt)) continue;
        if (x.chain_guard && !chain_guard_ok(x.chain_guard, C, cmax)) continue;
        pick = &x;
        break;
    }
    if (!pick)
        for (const auto &x : kVariants)
            if (x.gmem && actual_dc <= x.dc && !(force && *force && strncmp(x.name, force, strlen(force)) != 0)) {
                pick = &x;
                break;
            }
    if (!pick) return fail(FPLDPC_ERR_UNSUPPORTED, "no kernel variant for this code");
    const size_t lds = variant_lds(*pick, code);
    int dev = device;
    if (dev < 0) {
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
    }
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    // a kernel's static LDS would come out of the same 160 KiB (none of the kernels has any today: the
    // int32 kernels' block-wide OR goes through their control words, fpldpc_flood_int32.hpp block_or)
    hipFuncAttributes fattr;
    e = hipFuncGetAttributes(&fattr, (const void *)pick->fn);
    if (e != hipSuccess) return fail_hip(e, "hipFuncGetAttributes");
    if (lds + fattr.sharedSizeBytes > 160 * 1024)
        return fail(FPLDPC_ERR_UNSUPPORTED, "code length too large for LDS-resident posteriors and the kernel's static LDS");
    if (lds > 64 * 1024) {
        e = hipFuncSetAttribute((const void *)pick->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail_hip(e, "hipFuncSetAttribute");
    }
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pick->fn, pick->nt, lds);
    if (e != hipSuccess) return fail_hip(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (per_cu < 1) return fail(FPLDPC_ERR_UNSUPPORTED, "kernel cannot be resident (occupancy 0)");
    // Diagnostic: FPLDPC_GRID_PER_CU=k caps the persistent grid at k workgroups per CU (A/B runs)
    if (const char *g = getenv("FPLDPC_GRID_PER_CU"))
        if (atoi(g) > 0) per_cu = std::min(per_cu, atoi(g));
    out->v = pick->v;
    out->threads = pick->nt;
    out->grid = per_cu * prop.multiProcessorCount;
    out->fallback = pick->fallback;
    const int m_pad = (code.m + 63) / 64 * 64;
    out->scratch_ints = pick->gmem ? (size_t)out->grid * pick->dc * m_pad : (size_t)out->grid * pick->stat_words;
    // a fallback kernel: rare work, so one workgroup per CU is plenty and exits fast when empty
    auto setup_fallback = [&](Variant v, int *grid, int *threads, size_t *lds_out) -> int {
        const VariantInfo *fb = find_variant(v);
        const size_t fb_lds = variant_lds(*fb, code);
        if (fb_lds > 64 * 1024) {
            e = hipFuncSetAttribute((const void *)fb->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fb_lds);
            if (e != hipSuccess) return fail_hip(e, "hipFuncSetAttribute");
        }
        int fb_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&fb_cu, fb->fn, fb->nt, fb_lds);
        if (e != hipSuccess) return fail_hip(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
        if (fb_cu < 1) return fail(FPLDPC_ERR_UNSUPPORTED, "fallback kernel cannot be resident");
        *grid = prop.multiProcessorCount;
        *threads = fb->nt;
        *lds_out = fb_lds;
        if (fb->gmem) out->scratch_ints = std::max(out->scratch_ints, (size_t)*grid * fb->dc * m_pad);
        return FPLDPC_OK;
    };
    if (pick->fallback != Variant::kNone) {
        int st = setup_fallback(pick->fallback, &out->fb_grid, &out->fb_threads, &out->fb_lds);
        if (st) return st;
        const VariantInfo *fb = find_variant(pick->fallback);
        if (fb->fallback != Variant::kNone) {  // e.g. packed R kernel -> LDS-state int16 -> global int32
            out->fallback2 = fb->fallback;
            st = setup_fallback(fb->fallback, &out->fb2_grid, &out->fb2_threads, &out->fb2_lds);
            if (st) return st;
        }
        out->cmax = cmax;  // (packed_cmax)
    }
    out->lds_bytes = lds;
    out->name = pick->name;
    out->sort_checks = pick->lo_passes > 0;
    return FPLDPC_OK;
}

int launch_decode(const KernelChoice &kc, const DeviceCode &dcode, const LaunchArgs &la, void *stream) {
    const VariantInfo *vi = find_variant(kc.v);
    if (!vi) return fail(FPLDPC_ERR_ARG, "decoder has no kernel");
    if (la.batch <= 0) return FPLDPC_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    // A launch that fails leaves the counter block for the next call to find non-zero: re-zero it.
    auto launch_failed = [&](hipError_t err, const char *what) {
        (void)hipMemsetAsync(la.work_counter, 0, kCounterInts * sizeof(int32_t), s);
        return fail_hip(err, what);
    };
    KArgs a{};
    a.counters = la.work_counter;
    a.llr = la.llr;
    a.llr_i16 = la.llr_i16;
    a.n = dcode.n;
    a.m = dcode.m;
    a.m_pad = dcode.m_pad;
    a.batch = la.batch;
    a.max_iter = la.max_iter;
    a.C = la.C;
    a.mask = la.mask;
    a.early_term = la.early_term;
    a.precheck = la.precheck;
    a.vidx = dcode.vidx;
    a.cdeg = dcode.cdeg;
    a.hard = la.hard;
    a.hard_words = la.hard_words;
    a.iters = la.iters;
    a.syn_ok = la.syn_ok;
    a.post = la.post;
    a.bit_errors = la.bit_errors;
    a.totals = la.totals;
    a.info_idx = la.info_idx;
    a.info_bits = la.info_bits;
    a.k_info = la.k_info;
    a.info_mask = la.info_mask;
    a.work_counter = la.work_counter;
    a.c2v_scratch = la.c2v_scratch;
    a.bfe_w = la.bfe_w;
    a.probe = la.probe;
    a.wgtrace = la.wgtrace;
    a.split_tail = la.split_tail;
    if (kc.fallback == Variant::kNone) {
        const int grid = std::min(kc.grid, la.batch);
        a.last_in_chain = 1;
        hipLaunchKernelGGL(vi->fn, dim3(grid), dim3(kc.threads), kc.lds_bytes, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return launch_failed(e, "kernel launch");
        return FPLDPC_OK;
    }
    // packed kernel (two frames per workgroup), then the exact kernels of the fallback chain over
    // the frames each one rejected.  Counters: [0] work, [1] fallback work, [2] list-0 count,
    // [3] second fallback work, [4] list-1 count; list l is fb_list + l * batch.
    if (!la.fb_list) return fail(FPLDPC_ERR_ARG, "packed kernel needs a fallback list");
    int *const c = la.work_counter;
    a.fb_list = la.fb_list;
    a.fb_count = c + 2;
    a.cmax = kc.cmax;
    // The stationary exit is on when the kernel gets its scratch (a slice of stat_words per workgroup
    // of kc.grid, which no launch exceeds).  Its exit count rides in the list-1 size word, so the chain
    // must be one without a second list.
    if (vi->stat_words && !(la.stationary_exit && kc.fallback2 == Variant::kNone)) a.c2v_scratch = nullptr;
    const int per_wg = vi->lds_state ? 1 : 2;  // frames in flight per workgroup
    const int grid = std::min(kc.grid, (la.batch + per_wg - 1) / per_wg);
    // The cycle exit of the split tail shares that scratch, and its counter word counts the grid's workgroups
    // out in kCycOutBits bits.
    if (vi->stat_words && a.c2v_scratch && a.split_tail && la.cycle_exit && grid < (1 << kCycOutBits)) a.split_tail |= 2;
    hipLaunchKernelGGL(vi->fn, dim3(grid), dim3(kc.threads), kc.lds_bytes, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return launch_failed(e, "kernel launch");
    KArgs b = a;
    b.c2v_scratch = la.c2v_scratch;
    b.last_in_chain = kc.fallback2 == Variant::kNone;
    b.frame_list = la.fb_list;
    b.frame_count = c + 2;
    b.work_counter = c + 1;
    b.fb_list = kc.fallback2 != Variant::kNone ? la.fb_list + la.batch : nullptr;
    b.fb_count = kc.fallback2 != Variant::kNone ? c + 4 : nullptr;
    const VariantInfo *fb = find_variant(kc.fallback);
    hipLaunchKernelGGL(fb->fn, dim3(std::min(kc.fb_grid, la.batch)), dim3(kc.fb_threads), kc.fb_lds, s, b);
    e = hipGetLastError();
    if (e != hipSuccess) return launch_failed(e, "fallback kernel launch");
    if (kc.fallback2 == Variant::kNone) return FPLDPC_OK;
    KArgs b2 = b;
    b2.last_in_chain = 1;
    b2.frame_list = la.fb_list + la.batch;
    b2.frame_count = c + 4;
    b2.work_counter = c + 3;
    b2.fb_list = nullptr;
    b2.fb_count = nullptr;
    const VariantInfo *fb2 = find_variant(kc.fallback2);
    hipLaunchKernelGGL(fb2->fn, dim3(std::min(kc.fb2_grid, la.batch)), dim3(kc.fb2_threads), kc.fb2_lds, s, b2);
    e = hipGetLastError();
    if (e != hipSuccess) return launch_failed(e, "second fallback kernel launch");
    return FPLDPC_OK;
}

int edge_kernel_dc(int dc_max) {
    for (int d : {8, 16, 32, 48, 64})
        if (dc_max <= d) return d;
    return 0;
}

int launch_decode_frame(const LaunchArgs &la, const EdgeTables &t, int32_t *edge, int keep, void *stream) {
    KArgs a{};
    a.llr = la.llr;
    a.llr_i16 = la.llr_i16;
    a.n = t.n;
    a.m = t.m;
    a.batch = 1;
    a.max_iter = la.max_iter;
    a.C = la.C;
    a.mask = la.mask;
    a.early_term = la.early_term;
    a.precheck = la.precheck;
    a.hard = la.hard;
    a.hard_words = la.hard_words;
    a.iters = la.iters;
    a.syn_ok = la.syn_ok;
    a.post = la.post;
    const EdgeArgs e{t.vidx, t.cdeg, edge, t.c2v, keep, t.dc_max};
    size_t lds = (size_t)(4 * t.n + kMiscInts) * sizeof(int);
    if (lds > 160 * 1024) return fail(FPLDPC_ERR_UNSUPPORTED, "code length too large for LDS-resident posteriors");
    // the c2v double buffer [2][dc][m] int32 and the index table [dc][m] uint16 in LDS when they fit
    const size_t lds_state = lds + (size_t)t.dc * t.m * (2 * sizeof(int32_t) + sizeof(uint16_t));
    const bool in_lds = lds_state <= 160 * 1024 && !getenv("FPLDPC_EDGES_GLOBAL");
    if (in_lds) lds = lds_state;
    void (*fn)(KArgs, EdgeArgs) = nullptr;
    switch (t.dc) {
        case 8: fn = in_lds ? flood_edges<8, true> : flood_edges<8, false>; break;
        case 16: fn = in_lds ? flood_edges<16, true> : flood_edges<16, false>; break;
        case 32: fn = in_lds ? flood_edges<32, true> : flood_edges<32, false>; break;
        case 48: fn = in_lds ? flood_edges<48, true> : flood_edges<48, false>; break;
        case 64: fn = in_lds ? flood_edges<64, true> : flood_edges<64, false>; break;
        default: return fail(FPLDPC_ERR_UNSUPPORTED, "check degree above 64");
    }
    hipError_t err;
    if (lds > 64 * 1024) {
        err = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return fail_hip(err, "hipFuncSetAttribute");
    }
    hipLaunchKernelGGL(fn, dim3(1), dim3(kNT), lds, (hipStream_t)stream, a, e);
    err = hipGetLastError();
    if (err != hipSuccess) return fail_hip(err, "edge-state kernel launch");
    return FPLDPC_OK;
}

}  // namespace fpldpc

// Test-only (include/fpldpc_testing.h): the range parameters choose_kernel derives, without a device.
extern "C" uint32_t fpldpc_testing_range_guard(int32_t dv_max, int32_t C, int32_t slots, int32_t *chain_guard) {
    fpldpc_code code;
    code.dv_max = dv_max;
    const uint32_t cmax = fpldpc::packed_cmax(code, C);
    if (chain_guard) *chain_guard = cmax > 0 && fpldpc::chain_guard_ok(slots, C, cmax);
    return cmax;
}
