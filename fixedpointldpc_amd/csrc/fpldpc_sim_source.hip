// fpldpc_sim_source.hip -- the per-frame source of a BER simulation (fpldpc_sim_params.random_info): the
// information-bit stream, on the host and on the device, and the count of a decoded frame's information
// bits against the bits that frame was sent with.  Between them run the encoder and the channel of
// fpldpc_gen.hip; this unit is outside the kernel build id, as the layered and min-sum units are.  It also holds
// the forced positions of the float simulation (fpldpc_float_ber_sim), a kernel the hashed units do not have.
//
// Stream: the reference's Lehmer generator (rngs.cpp:40-69, a = 48271, m = 2^31 - 1) from info_seed, apart
// from the noise stream.  Bit i < k of frame f is the top bit of the 31-bit state after draw f*k + i, that
// is "uniform >= 1/2": (fpldpc_rng_skip(info_seed, f*k + i + 1) >> 30) & 1.  out[frames][k] is contiguous
// and so are its draws, so both forms walk one flat index j = (f - first_frame)*k + i.
#include <hip/hip_runtime.h>

#include "fpldpc_internal.hpp"
#include "fpldpc_sim_source.hpp"

namespace fpldpc {
namespace {

constexpr uint64_t kMod = 2147483647ull;  // rngs.cpp:40
constexpr uint64_t kMul = 48271ull;       // rngs.cpp:41
constexpr int kRun = 16;                  // consecutive draws per thread
constexpr int kPowBits = 48;              // draw indices < 2^48, the device channel's limit (fpldpc_gen.hip)
constexpr int kCountThreads = 256;        // count kernel: one wave per frame
constexpr int kWave = 64;

struct InfoArgs {
    uint64_t apow[kPowBits];  // a^(2^j) mod m
    uint64_t seed;
    uint64_t first_draw;  // first_frame * k
    int64_t total;        // frames * k
    uint8_t *out;
};

__device__ __forceinline__ uint64_t mulmod(uint64_t x, uint64_t y) {  // x, y < 2^31
    const uint64_t p = x * y;                                          // < 2^62
    uint64_t r = (p & kMod) + (p >> 31);                               // Mersenne fold
    r = (r & kMod) + (r >> 31);
    return r >= kMod ? r - kMod : r;
}

__global__ void __launch_bounds__(256) info_bits_kernel(InfoArgs a) {
    const int64_t j0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kRun;
    if (j0 >= a.total) return;
    // state after D draws = seed * a^D
    uint64_t D = a.first_draw + (uint64_t)j0;
    uint64_t s = a.seed;
#pragma unroll 1
    for (int j = 0; D; ++j, D >>= 1)
        if (D & 1) s = mulmod(s, a.apow[j]);
    const int64_t j1 = min(a.total, j0 + kRun);
    for (int64_t j = j0; j < j1; ++j) {
        s = mulmod(s, kMul);
        a.out[j] = (uint8_t)(s >> 30);  // s < 2^31
    }
}

// blkerror[f] = #{ i < k : bit info_idx[i] of hard[f] != info[f][i] }; wave w of a workgroup takes frame
// blockIdx.x * waves + w, its lanes stride over i
__global__ void __launch_bounds__(kCountThreads) count_info_kernel(const uint32_t *hard, int hard_words,
                                                                   const int32_t *info_idx, const uint8_t *info, int k,
                                                                   int frames, int32_t *blkerror) {
    const int lane = threadIdx.x % kWave;
    const int64_t f = (int64_t)blockIdx.x * (kCountThreads / kWave) + threadIdx.x / kWave;
    if (f >= frames) return;  // the whole wave: no barrier below
    const uint32_t *h = hard + (size_t)f * hard_words;
    const uint8_t *u = info + (size_t)f * k;
    int cnt = 0;
    for (int i = lane; i < k; i += kWave) {
        const int v = info_idx[i];
        cnt += (int)((h[v >> 5] >> (v & 31)) & 1u) != (int)(u[i] & 1u);
    }
    for (int off = kWave / 2; off; off >>= 1) cnt += __shfl_xor(cnt, off, kWave);
    if (lane == 0) blkerror[f] = cnt;
}

// The float simulation's forced positions: force_llr_kernel (fpldpc_gen.hip) on a double LLR array, one thread per
// (frame, forced position)
__global__ void __launch_bounds__(256) force_llr_f64_kernel(double *llr, int frames, int n, const int32_t *idx, int n_idx,
                                                            double value) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)frames * n_idx) return;
    llr[(t / n_idx) * n + idx[t % n_idx]] = value;
}

int info_args_ok(int64_t info_seed, int64_t first_frame, int32_t frames, int32_t k, const void *out) {
    if (info_seed < 1 || info_seed > (int64_t)kMod - 1) return fail(FPLDPC_ERR_ARG, "info_seed must be in 1 .. 2^31 - 2");
    if (k < 1 || frames < 0 || first_frame < 0 || (frames > 0 && !out)) return fail(FPLDPC_ERR_ARG, "bad info_bits arguments");
    const uint64_t lim = 1ull << kPowBits;
    // draws first_frame*k .. (first_frame + frames)*k - 1, and the state after the last one
    if ((uint64_t)first_frame >= lim || (uint64_t)first_frame + (uint64_t)frames >= lim ||
        (unsigned __int128)((uint64_t)first_frame + (uint64_t)frames) * (uint64_t)k >= lim)
        return fail(FPLDPC_ERR_ARG, "info_bits: draw index at or above 2^48");
    return FPLDPC_OK;
}

}  // namespace

int launch_count_info(const uint32_t *hard, int hard_words, const int32_t *info_idx, const uint8_t *info, int k,
                      int frames, int32_t *blkerror, void *stream) {
    if (frames <= 0) return FPLDPC_OK;
    const int per = kCountThreads / kWave;
    hipLaunchKernelGGL(count_info_kernel, dim3((unsigned)((frames + per - 1) / per)), dim3(kCountThreads), 0,
                       (hipStream_t)stream, hard, hard_words, info_idx, info, k, frames, blkerror);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : fail_hip((int)e, "count kernel launch");
}

int launch_force_llr_f64(double *llr, int frames, int n, const int32_t *idx, int n_idx, double value, void *stream) {
    const int64_t t = (int64_t)frames * n_idx;
    if (t <= 0) return FPLDPC_OK;
    hipLaunchKernelGGL(force_llr_f64_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, (hipStream_t)stream, llr,
                       frames, n, idx, n_idx, value);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : fail_hip((int)e, "float force kernel launch");
}

}  // namespace fpldpc

extern "C" {

int fpldpc_info_bits_host(int64_t info_seed, int64_t first_frame, int32_t frames, int32_t k, uint8_t *out) {
    const int st = fpldpc::info_args_ok(info_seed, first_frame, frames, k, out);
    if (st) return st;
    const int64_t total = (int64_t)frames * k;
    if (total == 0) return FPLDPC_OK;
    uint64_t s = (uint64_t)fpldpc_rng_skip(info_seed, (uint64_t)first_frame * (uint64_t)k);
    for (int64_t j = 0; j < total; ++j) {
        s = s * fpldpc::kMul % fpldpc::kMod;
        out[j] = (uint8_t)(s >> 30);
    }
    return FPLDPC_OK;
}

int fpldpc_info_bits(int64_t info_seed, int64_t first_frame, int32_t frames, int32_t k, uint8_t *out_dev, void *stream) {
    using namespace fpldpc;
    const int st = info_args_ok(info_seed, first_frame, frames, k, out_dev);
    if (st) return st;
    InfoArgs a;
    a.total = (int64_t)frames * k;
    if (a.total == 0) return FPLDPC_OK;
    uint64_t x = kMul;
    for (int j = 0; j < kPowBits; ++j) {
        a.apow[j] = x;
        x = x * x % kMod;  // x < 2^31
    }
    a.seed = (uint64_t)info_seed;
    a.first_draw = (uint64_t)first_frame * (uint64_t)k;
    a.out = out_dev;
    const int64_t threads = (a.total + kRun - 1) / kRun;
    hipLaunchKernelGGL(info_bits_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : fail_hip((int)e, "info bits kernel launch");
}

}  // extern "C"
