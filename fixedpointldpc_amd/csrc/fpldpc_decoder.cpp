// fpldpc_decoder.cpp -- the flooding decoder object and the device decode entry points of the C ABI
// (include/fpldpc.h): what the kernels read and how they are launched, which is what the kernel build id
// hashes of the host side.  The entry points that read the object or stage host buffers are
// fpldpc_decoder_api.cpp's, outside the id.
//
// Replaces the reference's FP_Decoder state (ArrayLDPCMacro.h:121-176) by a device-resident
// description of the code (slot-major var-index table, check degrees) plus the kernel choice.
// There is no CPU decode path here: without a usable HIP device every decode call fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "fpldpc_host.hpp"
#include "fpldpc_host_plan.hpp"

using namespace fpldpc;

namespace {

void free_decoder(fpldpc_decoder *d) {
    if (!d) return;
    DeviceGuard g(d->device);
    (void)hipFree(d->d_vidx);
    (void)hipFree(d->d_cdeg);
    (void)hipFree(d->d_counter);
    (void)hipFree(d->d_scratch);
    (void)hipFree(d->d_fb_list);
    if (d->h_probe) (void)hipHostFree(d->h_probe);
    if (d->h_wgtrace) (void)hipHostFree(d->h_wgtrace);
    (void)hipFree(d->d_info_mask);
    (void)hipFree(d->edges.vidx);
    (void)hipFree(d->edges.cdeg);
    (void)hipFree(d->edges.c2v);
    (void)hipFree(d->d_edge_stage);
    if (d->h_edge_stage) (void)hipHostFree(d->h_edge_stage);
    free_float_state(d->fl);
    if (d->last_done) (void)hipEventDestroy(d->last_done);
    core_free(*d);
    delete d;
}

// fpldpc_decode_frame's index table in the code's own check order (clist order per check), built on
// first use: slot k of check c -> var, [dc_max][m]; c2v scratch [2][edge_kernel_dc][m].
int edge_tables(fpldpc_decoder *d) {
    fpldpc::EdgeTables &t = d->edges;
    if (t.vidx) return FPLDPC_OK;
    const fpldpc_code &c = d->code;
    const int dc = edge_kernel_dc(c.dc_max);
    if (!dc) return fail(FPLDPC_ERR_UNSUPPORTED, "check degree above 64");
    const plan::SlotTable s = plan::slot_table(c.m, c.dc_max, c.cdeg.data(), c.clist.data(), c.dc_max, c.m, nullptr, 0);
    fpldpc::EdgeTables n;
    n.n = c.n;
    n.m = c.m;
    n.dc = dc;
    n.dc_max = c.dc_max;
    hipError_t e = hipMalloc(&n.vidx, s.vidx.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(n.vidx, s.vidx.data(), s.vidx.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&n.cdeg, s.cdeg.size());
    if (e == hipSuccess) e = hipMemcpy(n.cdeg, s.cdeg.data(), s.cdeg.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&n.c2v, sizeof(int32_t) * 2 * (size_t)dc * c.m);
    if (e != hipSuccess) {
        (void)hipFree(n.vidx);
        (void)hipFree(n.cdeg);
        (void)hipFree(n.c2v);
        return fail_hip((int)e, "edge tables");
    }
    t = n;
    return FPLDPC_OK;
}

// kc: the kernel choice to use (a twin takes its source's), or null to choose one for the code and
// device (FPLDPC_KERNEL may force it); diag: read the diagnostic switches from the environment.
int create_decoder(const fpldpc_code *code, const fpldpc_params *params, const KernelChoice *kc, bool diag,
                   fpldpc_decoder_t *out) {
    if (!code || !out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_params p;
    int st = resolve_params(params, &p);
    if (st) return st;
    int dev = -1;
    st = select_device(p.device, &dev);
    if (st) return st;
    DeviceGuard g(dev);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");

    std::unique_ptr<fpldpc_decoder, void (*)(fpldpc_decoder *)> d(new fpldpc_decoder(), free_decoder);
    d->code = *code;
    d->params = p;
    d->device = dev;
    if (kc) {
        d->kc = *kc;
    } else {
        st = choose_kernel(d->code, dev, p.width_mask, constant_c(p.frac_bits), &d->kc);
        if (st) return st;
    }

    const fpldpc_code &c = d->code;
    const int DC = kernel_dc(d->kc.v);
    const int m_pad = (c.m + 63) / 64 * 64;
    // Slot-major var-index table: vidx[k][j] = clist[c][k] (fold order) for the check c in column j,
    // 0 in unused slots so that every gather stays in bounds.  Columns are the checks in code order,
    // or by ascending degree (stable) for variants whose first passes fold a fixed degree: the
    // decode does not depend on check order (each check folds its own edges; posterior sums are
    // integer adds).
    std::vector<int> order(c.m);
    for (int r = 0; r < c.m; r++) order[r] = r;
    if (d->kc.sort_checks)
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return c.cdeg[x] < c.cdeg[y]; });
    const plan::SlotTable t = plan::slot_table(c.m, c.dc_max, c.cdeg.data(), c.clist.data(), DC, m_pad, order.data(), 0);
    HIP_TRY(hipMalloc(&d->d_vidx, t.vidx.size() * sizeof(uint16_t)));
    HIP_TRY(hipMemcpy(d->d_vidx, t.vidx.data(), t.vidx.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&d->d_cdeg, t.cdeg.size()));
    HIP_TRY(hipMemcpy(d->d_cdeg, t.cdeg.data(), t.cdeg.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&d->d_counter, kCounterInts * sizeof(int32_t)));  // zero between calls (chain_exit)
    HIP_TRY(hipMemset(d->d_counter, 0, kCounterInts * sizeof(int32_t)));
    if (d->kc.scratch_ints) HIP_TRY(hipMalloc(&d->d_scratch, d->kc.scratch_ints * sizeof(int32_t)));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&d->last_done, hipEventDisableTiming));
    d->dcode.n = c.n;
    d->dcode.m = c.m;
    d->dcode.dc = DC;
    d->dcode.m_pad = m_pad;
    d->dcode.vidx = d->d_vidx;
    d->dcode.cdeg = d->d_cdeg;
    // Diagnostics, read once here rather than on every decode call (see fpldpc_decode)
    if (const char *sp = getenv("FPLDPC_SPLIT_TAIL")) d->split_tail = *sp != '0';
    if (const char *se = getenv("FPLDPC_STATIONARY_EXIT")) d->stationary_exit = *se != '0';
    if (const char *ce = getenv("FPLDPC_CYCLE_EXIT")) d->cycle_exit = *ce != '0';
    if (diag) {
        const char *probe_env = getenv("FPLDPC_CLOCK_PROBE");
        d->diag_probe = probe_env && *probe_env == '1';
        if (const char *t = getenv("FPLDPC_WG_TRACE")) d->diag_trace_path = t;
    }
    *out = d.release();
    return FPLDPC_OK;
}

// The launch arguments fpldpc_decode and fpldpc_decode_frame have in common.
LaunchArgs launch_args(const fpldpc_decoder &dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                       int32_t *iters, uint8_t *syndrome_ok, int32_t *post) {
    LaunchArgs a;
    a.llr = llr;
    a.llr_i16 = llr_type == FPLDPC_LLR_I16;
    a.batch = batch;
    a.max_iter = dec.params.max_iter;
    a.C = constant_c(dec.params.frac_bits);
    a.mask = dec.params.width_mask;
    a.early_term = dec.params.early_term;
    a.precheck = dec.params.precheck;
    a.hard = hard;
    a.hard_words = (dec.code.n + 31) / 32;
    a.iters = iters;
    a.syn_ok = syndrome_ok;
    a.post = post;
    return a;
}

}  // namespace

namespace fpldpc {
int decoder_create_twin(fpldpc_decoder_t src, fpldpc_decoder_t *out) {
    if (!src) return fail(FPLDPC_ERR_ARG, "null decoder");
    fpldpc_params p = src->params;
    p.device = src->device;
    return create_decoder(&src->code, &p, &src->kc, false, out);
}
}  // namespace fpldpc

extern "C" {

int fpldpc_decoder_create(fpldpc_code_t code, const fpldpc_params *params, fpldpc_decoder_t *out) {
    return create_decoder(code, params, nullptr, true, out);
}

int fpldpc_decoder_destroy(fpldpc_decoder_t dec) {
    free_decoder(dec);
    return FPLDPC_OK;
}

// The core's reference bits, and beside them the packed mask the packed kernels count from.  On every return
// d_info_mask is set only beside k_info > 0, and is then the mask of exactly the uploaded reference.
int fpldpc_set_reference(fpldpc_decoder_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k) {
    const int st = set_reference(dec, info_index, info_bits, k);
    if (!dec || (st && dec->k_info > 0)) return st;  // refused arguments: the previous reference stands, mask included
    DeviceGuard g(dec->device);
    (void)hipFree(dec->d_info_mask);
    dec->d_info_mask = nullptr;
    if (st || k == 0) return st;
    const std::vector<uint32_t> mk = plan::reference_mask(dec->code.n, info_index, info_bits, k);
    if (mk.empty()) return FPLDPC_OK;  // a position repeats: the kernels count from the index form
    hipError_t e = hipMalloc(&dec->d_info_mask, mk.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(dec->d_info_mask, mk.data(), mk.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) return FPLDPC_OK;
    (void)hipFree(dec->d_info_mask);
    dec->d_info_mask = nullptr;
    (void)set_reference(dec, nullptr, nullptr, 0);  // as any failed upload: no reference
    return fail_hip((int)e, "reference mask");
}

int fpldpc_decode(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                  int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                  void *stream) {
    DeviceGuard g;
    bool run = false;
    int st = decode_prologue(dec, llr, &llr_type, batch, bit_errors, "fpldpc_set_reference", &g, &run);
    if (st || !run) return st;
    LaunchArgs a = launch_args(*dec, llr, llr_type, batch, hard, iters, syndrome_ok, post);
    a.bit_errors = bit_errors;
    a.totals = reinterpret_cast<unsigned long long *>(totals);
    a.info_idx = dec->d_info_idx;
    a.info_bits = dec->d_info_bits;
    a.k_info = dec->k_info;
    a.info_mask = dec->d_info_mask;
    a.work_counter = dec->d_counter;
    a.c2v_scratch = dec->d_scratch;
    a.bfe_w = (uint32_t)std::max(0, __builtin_popcount((unsigned)a.mask) - 2);
    a.split_tail = dec->split_tail ? 1 : 0;
    a.stationary_exit = dec->stationary_exit ? 1 : 0;
    a.cycle_exit = dec->cycle_exit ? 1 : 0;
    if (dec->kc.fallback != Variant::kNone) {
        if (batch > dec->fb_cap) {  // grows to the largest batch seen (not inside graph capture)
            (void)hipFree(dec->d_fb_list);
            dec->d_fb_list = nullptr;
            dec->fb_cap = 0;
            HIP_TRY(hipMalloc(&dec->d_fb_list, sizeof(int) * (size_t)batch * dec->kc.lists()));
            dec->fb_cap = batch;
        }
        a.fb_list = dec->d_fb_list;
    }
    // Diagnostic: FPLDPC_CLOCK_PROBE=1 (at decoder creation) stamps workgroup 0's shader clock
    // (s_memtime) against the 100 MHz s_memrealtime around the kernel and prints the in-kernel clock
    // (synchronises).
    const bool probe = dec->diag_probe;
    if (probe && !dec->h_probe) HIP_TRY(hipHostMalloc((void **)&dec->h_probe, 64, hipHostMallocMapped));
    if (probe) {
        memset(dec->h_probe, 0, 64);
        a.probe = dec->h_probe;
    }
    // Diagnostic: FPLDPC_WG_TRACE=<file> (at decoder creation) writes, after each call, every
    // workgroup's {xcc<<32 | HW_ID, start, end (100 MHz s_memrealtime), frames pulled, 4 reserved
    // words} of the packed kernels as raw uint64 [grid][8].
    const char *trace_path = dec->diag_trace_path.empty() ? nullptr : dec->diag_trace_path.c_str();
    if (trace_path) {
        // [grid][8] per workgroup, then [grid][64] per wave (the FPLDPC_WAIT_TRACE diagnostic build)
        if (!dec->h_wgtrace)
            HIP_TRY(hipHostMalloc((void **)&dec->h_wgtrace, sizeof(unsigned long long) * 72 * dec->kc.grid, hipHostMallocMapped));
        memset(dec->h_wgtrace, 0, sizeof(unsigned long long) * 72 * dec->kc.grid);
        a.wgtrace = dec->h_wgtrace;
    }
    st = launch_decode(dec->kc, dec->dcode, a, stream);
    if (!st && dec->kc.fallback != Variant::kNone) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &cs));
        if (cs == hipStreamCaptureStatusNone) HIP_TRY(hipEventRecord(dec->last_done, (hipStream_t)stream));
    }
    if (!st && a.wgtrace) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (FILE *f = fopen(trace_path, "wb")) {
            fwrite(dec->h_wgtrace, sizeof(unsigned long long), 8 * (size_t)dec->kc.grid, f);
            fclose(f);
        }
        const unsigned long long *w = dec->h_wgtrace + 8 * (size_t)dec->kc.grid;
        if (std::any_of(w, w + 64 * (size_t)dec->kc.grid, [](unsigned long long x) { return x != 0; }))
            if (FILE *f = fopen((dec->diag_trace_path + ".waves").c_str(), "wb")) {
                fwrite(w, sizeof(unsigned long long), 64 * (size_t)dec->kc.grid, f);
                fclose(f);
            }
    }
    if (st || !probe) return st;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const unsigned long long *q = dec->h_probe;
    if (q[2] > q[0] && q[3] > q[1])
        fprintf(stderr, "fpldpc clock probe: %.0f MHz (workgroup 0: %llu cycles in %.3f ms)\n",
                (double)(q[2] - q[0]) / (double)(q[3] - q[1]) * 100.0, q[2] - q[0], (q[3] - q[1]) * 1e-5);
    return st;
}

int fpldpc_decode_frame(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t keep_edges, int32_t *edge_ram,
                        uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok, int32_t *post, void *stream) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (!llr || !edge_ram) return fail(FPLDPC_ERR_ARG, "null llr or edge RAM");
    if (llr_type != FPLDPC_LLR_I32 && llr_type != FPLDPC_LLR_I16) return fail(FPLDPC_ERR_ARG, "bad llr_type");
    DeviceGuard g(dec->device);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    const int st = edge_tables(dec);
    if (st) return st;
    return launch_decode_frame(launch_args(*dec, llr, llr_type, 1, hard, iters, syndrome_ok, post), dec->edges, edge_ram,
                               keep_edges != 0, stream);
}

}  // extern "C"
