// fpldpc_harvest.hip -- the harvest of a BER simulation (include/fpldpc.h, fpldpc_harvest_t): for every
// decoded frame the error pattern e = hard XOR sent word and the syndrome of the hard decision, their weights
// (a, b), and the ordered compaction of a chunk's codeword-error frames into a record buffer.  This unit is
// outside the kernel build id, as the layered, min-sum and simulation-source units are.
//
// Scan: a wave per frame, four frames per workgroup.  The wave stages its frame's hard words in LDS (tail word
// masked to n bits), then walks the variables 64 at a time -- a lane per codeword byte, __ballot packs the
// 64 bits, XOR with two staged words, popcount -- and the checks 64 at a time: a lane per check folds its
// variables' bits from LDS through a table uint16 [dc][m] (consecutive lanes read consecutive entries; a slot
// past a check's degree holds kHarvestPad), __ballot packs the syndrome.  Every store is a vector store by the
// lane that owns the word; nothing is ordered by an atomic.
//
// Compaction: pos[f] = number of frames before f with weight > 0 (one workgroup, ballot prefix per wave and a
// running carry over tiles of 256 frames), -1 where weight is 0 or the index is at or above the buffer's
// capacity; then a wave per frame copies the row of a frame with pos >= 0 to record pos.  The records are the
// first `cap` codeword-error frames in frame order whatever the order the workgroups run in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "fpldpc_harvest.hpp"
#include "fpldpc_testing.h"

namespace fpldpc {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kPer = kThreads / kWave;  // frames per workgroup
constexpr int kAhead = 4;               // scan: 64-variable steps whose codeword bytes are loaded together
constexpr int kSlots = 8;               // scan: slots of a check whose table entries are loaded together

struct ScanArgs {
    const uint32_t *hard;
    const uint8_t *cw;
    const uint16_t *table;
    int32_t *weight, *unsat;
    uint32_t *err, *syn;
    int n, m, dc, hard_words, syn_words, stage_words;  // stage_words: hard_words rounded up to even
    int batch, cw_per_frame, err_pitch, syn_pitch;
};

__global__ void __launch_bounds__(kThreads) harvest_scan_kernel(ScanArgs a) {
    extern __shared__ uint32_t staged[];  // [kPer][stage_words]
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t f = (int64_t)blockIdx.x * kPer + wave;
    const bool live = f < a.batch;
    uint32_t *h = staged + (size_t)wave * a.stage_words;
    if (live) {
        const uint32_t *src = a.hard + (size_t)f * a.hard_words;
        const uint32_t tail = a.n % 32 ? (1u << (a.n % 32)) - 1u : 0xffffffffu;
        for (int i = lane; i < a.stage_words; i += kWave) {
            uint32_t v = i < a.hard_words ? src[i] : 0u;
            if (i == a.hard_words - 1) v &= tail;  // bits at or above n are ignored, whatever they hold
            h[i] = v;
        }
    }
    __syncthreads();
    if (!live) return;  // the whole wave: no barrier below
    const uint8_t *c = a.cw ? a.cw + (a.cw_per_frame ? (size_t)f * a.n : 0) : nullptr;
    int weight = 0;
    for (int b0 = 0; b0 * kWave < a.n; b0 += kAhead) {
        uint32_t byte[kAhead];  // kAhead steps' loads in flight before the first ballot waits for one
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int v = (b0 + j) * kWave + lane;
            byte[j] = c && v < a.n ? c[v] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int b = b0 + j;
            if (b * kWave >= a.n) break;  // the whole wave
            const unsigned long long sent = __ballot(byte[j] & 1u);
            const unsigned long long e = (h[2 * b] | (unsigned long long)h[2 * b + 1] << 32) ^ sent;
            weight += __popcll(e);
            if (a.err && lane < 2 && 2 * b + lane < a.hard_words)
                a.err[(size_t)f * a.err_pitch + 2 * b + lane] = (uint32_t)(e >> (32 * lane));
        }
    }
    int unsat = 0;
    for (int b = 0; b * kWave < a.m; ++b) {
        const int chk = b * kWave + lane;
        uint32_t par = 0;
        if (chk < a.m)
            for (int k0 = 0; k0 < a.dc; k0 += kSlots) {
                uint32_t v[kSlots];  // kSlots table loads in flight before the first LDS read waits for one
#pragma unroll
                for (int j = 0; j < kSlots; ++j) v[j] = k0 + j < a.dc ? a.table[(size_t)(k0 + j) * a.m + chk] : kHarvestPad;
#pragma unroll
                for (int j = 0; j < kSlots; ++j)
                    if (v[j] != kHarvestPad) par ^= h[v[j] >> 5] >> (v[j] & 31);
            }
        const unsigned long long s = __ballot(par & 1u);
        unsat += __popcll(s);
        if (a.syn && lane < 2 && 2 * b + lane < a.syn_words)
            a.syn[(size_t)f * a.syn_pitch + 2 * b + lane] = (uint32_t)(s >> (32 * lane));
    }
    if (lane == 0) {
        a.weight[f] = weight;
        a.unsat[f] = unsat;
    }
}

__global__ void __launch_bounds__(kThreads) harvest_index_kernel(const int32_t *weight, int batch, int cap, int32_t *pos) {
    __shared__ int wave_sum[kPer];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int carry = 0;  // codeword-error frames before this tile
    for (int base = 0; base < batch; base += kThreads) {
        const int f = base + threadIdx.x;
        const bool flag = f < batch && weight[f] > 0;
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) wave_sum[wave] = __popcll(mask);
        __syncthreads();
        int before = carry, tile = 0;
        for (int i = 0; i < kPer; ++i) {
            if (i < wave) before += wave_sum[i];
            tile += wave_sum[i];
        }
        const int p = before + __popcll(mask & ((1ull << lane) - 1ull));
        if (f < batch) pos[f] = flag && p < cap ? p : -1;
        carry += tile;
        __syncthreads();  // wave_sum is rewritten by the next tile
    }
}

__global__ void __launch_bounds__(kThreads) harvest_gather_kernel(const int32_t *pos, const uint32_t *rows, int row_words,
                                                                  int batch, uint32_t *rec) {
    const int lane = threadIdx.x % kWave;
    const int64_t f = (int64_t)blockIdx.x * kPer + threadIdx.x / kWave;
    if (f >= batch) return;
    const int p = pos[f];
    if (p < 0) return;
    const uint32_t *src = rows + (size_t)f * row_words;
    uint32_t *dst = rec + (size_t)p * row_words;
    for (int i = lane; i < row_words; i += kWave) dst[i] = src[i];
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : fail_hip((int)e, what);
}

}  // namespace

int harvest_upload_table(const fpldpc_harvest &h, uint16_t **out) {
    std::vector<uint16_t> t((size_t)h.dc * h.m);
    for (int c = 0; c < h.m; ++c)
        for (int k = 0; k < h.dc; ++k) {
            const int32_t v = h.clist[(size_t)c * h.dc + k];
            t[(size_t)k * h.m + c] = v < 0 ? kHarvestPad : (uint16_t)v;
        }
    hipError_t e = hipMalloc((void **)out, t.size() * sizeof(uint16_t));
    if (e != hipSuccess) return fail_hip((int)e, "hipMalloc (harvest table)");
    e = hipMemcpy(*out, t.data(), t.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(*out);
        *out = nullptr;
        return fail_hip((int)e, "hipMemcpy (harvest table)");
    }
    return FPLDPC_OK;
}

int launch_harvest_scan(const fpldpc_harvest &h, const uint16_t *table, const uint32_t *hard, const uint8_t *cw,
                        int cw_per_frame, int batch, int32_t *weight, int32_t *unsat, uint32_t *err, int err_pitch,
                        uint32_t *syn, int syn_pitch, void *stream) {
    if (batch <= 0) return FPLDPC_OK;
    ScanArgs a;
    a.hard = hard;
    a.cw = cw;
    a.table = table;
    a.weight = weight;
    a.unsat = unsat;
    a.err = err;
    a.syn = syn;
    a.n = h.n;
    a.m = h.m;
    a.dc = h.dc;
    a.hard_words = h.hard_words;
    a.syn_words = h.syn_words;
    a.stage_words = (h.hard_words + 1) & ~1;
    a.batch = batch;
    a.cw_per_frame = cw_per_frame;
    a.err_pitch = err_pitch;
    a.syn_pitch = syn_pitch;
    hipLaunchKernelGGL(harvest_scan_kernel, dim3((unsigned)((batch + kPer - 1) / kPer)), dim3(kThreads),
                       sizeof(uint32_t) * kPer * a.stage_words, (hipStream_t)stream, a);
    return launched("harvest scan kernel launch");
}

int launch_harvest_compact(const int32_t *weight, const uint32_t *rows, int row_words, int batch, int cap, int32_t *pos,
                           uint32_t *rec, void *stream) {
    if (batch <= 0 || cap <= 0) return FPLDPC_OK;
    hipLaunchKernelGGL(harvest_index_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, weight, batch, cap, pos);
    if (const int st = launched("harvest index kernel launch")) return st;
    hipLaunchKernelGGL(harvest_gather_kernel, dim3((unsigned)((batch + kPer - 1) / kPer)), dim3(kThreads), 0,
                       (hipStream_t)stream, pos, rows, row_words, batch, rec);
    return launched("harvest gather kernel launch");
}

}  // namespace fpldpc

using namespace fpldpc;

fpldpc_harvest::~fpldpc_harvest() {
    if (d_table) (void)hipFree(d_table);
}

void fpldpc_harvest::clear() {
    std::fill(counts, counts + 6, (int64_t)0);
    full = max_records == 0;
    frame.clear();
    iters.clear();
    info_errors.clear();
    weight.clear();
    unsat.clear();
    err.clear();
    syn.clear();
    classes.clear();
}

void fpldpc_harvest::add_error_frame(int64_t f, int32_t its, int32_t blk, int32_t w, int32_t u, const uint32_t *row) {
    ++counts[1];
    ++counts[u > 0 ? 2 : 3];
    ++classes[(uint64_t)(uint32_t)w << 32 | (uint32_t)u];
    if (counts[4] >= max_records) {
        ++counts[5];
        return;
    }
    if (++counts[4] >= max_records) full = true;
    frame.push_back(f);
    iters.push_back(its);
    info_errors.push_back(blk);
    weight.push_back(w);
    unsat.push_back(u);
    err.insert(err.end(), row, row + hard_words);
    syn.insert(syn.end(), row + hard_words, row + hard_words + syn_words);
}

extern "C" {

int fpldpc_harvest_create(fpldpc_code_t code, int32_t max_records, fpldpc_harvest_t *out) {
    if (!code || !out) return fail(FPLDPC_ERR_ARG, "harvest: null argument");
    if (max_records < 0 || max_records > (1 << 20)) return fail(FPLDPC_ERR_ARG, "harvest: max_records must be in 0 .. 2^20");
    if (code->n < 1 || code->n > 65535 || code->m < 1 || code->dc_max < 1)
        return fail(FPLDPC_ERR_UNSUPPORTED, "harvest: n must be in 1 .. 65535");
    std::unique_ptr<fpldpc_harvest> h(new fpldpc_harvest());
    h->n = code->n;
    h->m = code->m;
    h->dc = code->dc_max;
    h->hard_words = (code->n + 31) / 32;
    h->syn_words = (code->m + 31) / 32;
    h->max_records = max_records;
    h->clist = code->clist;
    *out = h.release();
    return FPLDPC_OK;
}

void fpldpc_harvest_free(fpldpc_harvest_t h) { delete h; }

int fpldpc_harvest_scan(fpldpc_harvest_t h, const uint32_t *hard, const uint8_t *cw, int32_t cw_per_frame, int32_t batch,
                        int32_t *weight, int32_t *unsat, uint32_t *err, uint32_t *syn, void *stream) {
    if (!h || batch < 0 || (batch > 0 && (!hard || !weight || !unsat)) || (cw_per_frame != 0 && cw_per_frame != 1))
        return fail(FPLDPC_ERR_ARG, "harvest scan: bad argument");
    if (batch == 0) return FPLDPC_OK;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail_hip((int)e, "hipGetDevice");
    if (h->d_table && h->device != dev) return fail(FPLDPC_ERR_ARG, "harvest already bound to another device");
    if (!h->d_table) {
        const int st = harvest_upload_table(*h, &h->d_table);
        if (st) return st;
        h->device = dev;
    }
    return launch_harvest_scan(*h, h->d_table, hard, cw, cw_per_frame, batch, weight, unsat, err, h->hard_words, syn,
                               h->syn_words, stream);
}

int fpldpc_harvest_dims(fpldpc_harvest_t h, int32_t dims[4]) {
    if (!h || !dims) return fail(FPLDPC_ERR_ARG, "harvest: null argument");
    dims[0] = h->n;
    dims[1] = h->m;
    dims[2] = h->hard_words;
    dims[3] = h->syn_words;
    return FPLDPC_OK;
}

int fpldpc_harvest_counts(fpldpc_harvest_t h, int64_t counts[6]) {
    if (!h || !counts) return fail(FPLDPC_ERR_ARG, "harvest: null argument");
    std::copy(h->counts, h->counts + 6, counts);
    return FPLDPC_OK;
}

int fpldpc_harvest_records(fpldpc_harvest_t h, int64_t first, int64_t count, int64_t *frame, int32_t *iters,
                           int32_t *info_errors, int32_t *weight, int32_t *unsat, uint32_t *err, uint32_t *syn) {
    if (!h) return fail(FPLDPC_ERR_ARG, "harvest: null argument");
    const int64_t have = (int64_t)h->frame.size();
    if (first < 0 || count < 0 || first > have || count > have - first)
        return fail(FPLDPC_ERR_ARG, "harvest: records outside [0, recorded]");
    if (count == 0) return FPLDPC_OK;
    const size_t a = (size_t)first, c = (size_t)count;
    if (frame) memcpy(frame, h->frame.data() + a, c * sizeof(int64_t));
    if (iters) memcpy(iters, h->iters.data() + a, c * sizeof(int32_t));
    if (info_errors) memcpy(info_errors, h->info_errors.data() + a, c * sizeof(int32_t));
    if (weight) memcpy(weight, h->weight.data() + a, c * sizeof(int32_t));
    if (unsat) memcpy(unsat, h->unsat.data() + a, c * sizeof(int32_t));
    if (err) memcpy(err, h->err.data() + a * h->hard_words, c * h->hard_words * sizeof(uint32_t));
    if (syn) memcpy(syn, h->syn.data() + a * h->syn_words, c * h->syn_words * sizeof(uint32_t));
    return FPLDPC_OK;
}

int fpldpc_harvest_classes(fpldpc_harvest_t h, int32_t *weight, int32_t *unsat, int64_t *count, int32_t cap,
                           int32_t *n_classes) {
    if (!h || !n_classes || cap < 0) return fail(FPLDPC_ERR_ARG, "harvest: bad argument");
    *n_classes = (int32_t)h->classes.size();
    std::vector<std::pair<uint64_t, int64_t>> sorted(h->classes.begin(), h->classes.end());
    std::sort(sorted.begin(), sorted.end());  // the key's order: by weight, then by unsat
    for (int i = 0; i < cap && i < (int)sorted.size(); ++i) {
        if (weight) weight[i] = (int32_t)(sorted[i].first >> 32);
        if (unsat) unsat[i] = (int32_t)(sorted[i].first & 0xffffffffu);
        if (count) count[i] = sorted[i].second;
    }
    return FPLDPC_OK;
}

int fpldpc_testing_harvest_compact(const int32_t *weight, const uint32_t *rows, int32_t row_words, int32_t batch,
                                   int32_t cap, int32_t *pos, uint32_t *rec, void *stream) {
    if (batch < 0 || cap < 0 || row_words < 1 || (batch > 0 && cap > 0 && (!weight || !rows || !pos || !rec)))
        return fail(FPLDPC_ERR_ARG, "harvest compaction: bad argument");
    return launch_harvest_compact(weight, rows, row_words, batch, cap, pos, rec, stream);
}

}  // extern "C"
