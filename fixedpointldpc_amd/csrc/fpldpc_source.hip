// fpldpc_source.hip -- the counter-based noise source on the device (include/fpldpc.h, FPLDPC_NOISE_PHILOX): the
// Philox channel kernel, the patch kernel that a bias puts behind it, and the device entry points that take a
// source.  This unit is outside the kernel build id, as the bias, harvest, layered, min-sum and simulation-source
// units are; the Lehmer channel (fpldpc_gen.hip) and its patch kernel (fpldpc_bias.hip) are untouched and are
// reached through their own launchers.
//
// For frame f and the pair p = i >> 1 of position i, (r0 .. r3) = Philox4x32-10(counter (p, 0, f lo, f hi), key
// (seed lo, seed hi)) give u1 = ((r0 | r1 << 32) >> 11 + 1) * 2^-53 in (0, 1] and u2 = ((r2 | r3 << 32) >> 11) *
// 2^-53 in [0, 1); rad = sqrt(-2 ln u1), z = rad * cos(2 pi u2) at even i, rad * sin(2 pi u2) at odd i.  From z
// on the channel is channel_kernel's: nrm = 0.0 + sigma*z, LLR = (2*snr) * ((1 - 2c) + nrm), LLR_fp =
// (int)(LLR * 2^frac), each operation rounded once.  sincospi(2*u2) takes the exact 2*u2, so no reduction by pi.
//
// Channel kernel: one thread per pair, consecutive lanes on consecutive pairs of a frame (and on into the next
// frame), so that a wave's stores are contiguous; no table and no loop to reach a position.  With odd n the last
// pair's sine half is not stored.  One integer atomic per thread where its overflow count is not zero.
// Patch kernel: bias_patch_kernel's form (fpldpc_bias.hip) -- a wave per frame, lanes striding the biased
// positions, term_j summed per lane in ascending j, the xor butterfly in a fixed order, no floating-point atomic
// -- with the variate of position pos[j] from the Philox call of its pair, formed by the same inlined code as the
// channel kernel's, so that a zero shift writes back the channel's bits.  No LDS, no scratch in either.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fpldpc_source.hpp"

namespace fpldpc {
namespace {

constexpr int kWave = 64;
constexpr int kPer = 8;  // patch kernel: frames per workgroup
constexpr int kPatchThreads = kWave * kPer;
constexpr int kChanThreads = 256;

struct PhiloxArgs {
    uint64_t seed;
    int64_t first_frame;
    int frames, n, frac, out_type, cw_per_frame, count;
    double snr, sigma;
    const uint8_t *cw;
    const int32_t *pos;    // patch kernel only
    const double *shift;   // patch kernel only
    void *out;
    int *overflow;
    double *logw;          // patch kernel only
};

// (rad cos(2 pi u2), rad sin(2 pi u2)) of one pair
__device__ __forceinline__ void pair_variates(uint64_t seed, uint64_t frame, uint32_t pair, double *zc, double *zs) {
    double u1, u2, s, c;
    philox_uniforms(seed, frame, pair, &u1, &u2);
    const double rad = sqrt(__dmul_rn(-2.0, log(u1)));
    sincospi(__dmul_rn(2.0, u2), &s, &c);
    *zc = __dmul_rn(rad, c);
    *zs = __dmul_rn(rad, s);
}

// The same behind a call, for the patch kernel: inlined into its loop over the biased positions, the constants of
// log and sincospi are hoisted out of the loop into 34 VGPRs (94 in all, five waves per SIMD); behind a call they
// stay in the callee (53, eight waves), and the bits are those of the inlined form.
__device__ __noinline__ double2 pair_variates_call(uint64_t seed, uint64_t frame, uint32_t pair) {
    double2 r;
    pair_variates(seed, frame, pair, &r.x, &r.y);
    return r;
}

__global__ void __launch_bounds__(kChanThreads) philox_channel_kernel(PhiloxArgs a) {
    const uint32_t ppf = ((uint32_t)a.n + 1u) >> 1;  // pairs per frame
    const uint64_t tid = (uint64_t)blockIdx.x * kChanThreads + threadIdx.x;
    const uint64_t total = (uint64_t)a.frames * ppf;
    if (tid >= total) return;
    // most calls have fewer than 2^32 pairs: a 32-bit division then
    const uint32_t f = total >> 32 ? (uint32_t)(tid / ppf) : (uint32_t)tid / ppf;
    const uint32_t p = (uint32_t)(tid - (uint64_t)f * ppf);
    double z[2];
    pair_variates(a.seed, (uint64_t)a.first_frame + f, p, &z[0], &z[1]);
    const double scale = (double)(1 << a.frac);
    const double two_snr = __dmul_rn(2.0, a.snr);
    const uint8_t *cw = a.cw ? a.cw + (a.cw_per_frame ? (size_t)f * a.n : 0) : nullptr;
    const size_t base = (size_t)f * a.n;
    const int i0 = (int)(2u * p);
    int ovf = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = i0 + h;
        if (i >= a.n) break;  // odd n: the last pair's sine half
        const double nrm = __dadd_rn(0.0, __dmul_rn(a.sigma, z[h]));
        const int c = cw ? (int)(cw[i] & 1) : 0;
        const double llr = __dmul_rn(two_snr, __dadd_rn((double)(1 - 2 * c), nrm));
        if (a.out_type == FPLDPC_LLR_F64) {
            static_cast<double *>(a.out)[base + i] = llr;
            continue;
        }
        const int x = (int)__dmul_rn(llr, scale);  // (int) truncation, no clipping
        if (a.out_type == FPLDPC_LLR_I16) {
            ovf += (x < -32768) | (x > 32767);
            static_cast<int16_t *>(a.out)[base + i] = (int16_t)x;
        } else {
            static_cast<int32_t *>(a.out)[base + i] = x;
        }
    }
    if (ovf && a.overflow) atomicAdd(a.overflow, ovf);
}

__global__ void __launch_bounds__(kPatchThreads) philox_patch_kernel(PhiloxArgs a) {
    const int lane = threadIdx.x % kWave;
    const int64_t f = (int64_t)blockIdx.x * kPer + threadIdx.x / kWave;
    if (f >= a.frames) return;  // the whole wave
    const double scale = (double)(1 << a.frac);
    const uint8_t *cw = a.cw ? a.cw + (a.cw_per_frame ? (size_t)f * a.n : 0) : nullptr;
    const size_t base = (size_t)f * a.n;
    const uint64_t frame = (uint64_t)a.first_frame + (uint64_t)f;
    const double two_snr = __dmul_rn(2.0, a.snr);
    const double den = __dmul_rn(__dmul_rn(2.0, a.sigma), a.sigma);
    double sum = 0.0;
    int ovf = 0;
#pragma unroll 1
    for (int j = lane; j < a.count; j += kWave) {
        const int i = a.pos[j];
        const double sh = a.shift[j];
        const double2 zz = pair_variates_call(a.seed, frame, (uint32_t)i >> 1);
        const double zc = zz.x, zs = zz.y;
        const double nrm = __dadd_rn(0.0, __dmul_rn(a.sigma, i & 1 ? zs : zc));
        const int c = cw ? (int)(cw[i] & 1) : 0;
        const double sg = (double)(1 - 2 * c);
        const double llr = __dmul_rn(two_snr, __dadd_rn(__dmul_rn(sg, __dsub_rn(1.0, sh)), nrm));
        sum = __dadd_rn(sum, __ddiv_rn(__dmul_rn(sh, __dsub_rn(__dmul_rn(__dmul_rn(2.0, sg), nrm), sh)), den));
        if (a.out_type == FPLDPC_LLR_F64) {
            static_cast<double *>(a.out)[base + i] = llr;
            continue;
        }
        const int x = (int)__dmul_rn(llr, scale);  // (int) truncation, no clipping
        if (a.out_type == FPLDPC_LLR_I16) {
            const int x0 = (int)__dmul_rn(__dmul_rn(two_snr, __dadd_rn(sg, nrm)), scale);  // what the channel stored
            ovf += (int)((x < -32768) | (x > 32767)) - (int)((x0 < -32768) | (x0 > 32767));
            static_cast<int16_t *>(a.out)[base + i] = (int16_t)x;
        } else {
            static_cast<int32_t *>(a.out)[base + i] = x;
        }
    }
    if (ovf && a.overflow) atomicAdd(a.overflow, ovf);
    if (!a.logw) return;
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) sum = __dadd_rn(sum, __shfl_xor(sum, m, kWave));
    if (lane == 0) a.logw[f] = sum;
}

int hip_fail(hipError_t e, const char *what) { return fail_hip((int)e, what); }

PhiloxArgs args(const ChannelArgs &c, int n) {
    PhiloxArgs a{};
    a.seed = (uint64_t)c.seed;
    a.first_frame = c.first_frame;
    a.frames = c.frames;
    a.n = n;
    a.frac = c.frac_bits;
    a.out_type = c.out_type;
    a.cw_per_frame = c.cw_per_frame;
    a.snr = c.snr;
    a.sigma = c.sigma;
    a.cw = c.cw;
    a.out = c.out;
    a.overflow = c.overflow;
    return a;
}

int bad_source() { return fail(FPLDPC_ERR_ARG, "bad noise source (FPLDPC_NOISE_LEHMER or FPLDPC_NOISE_PHILOX)"); }

}  // namespace

int launch_channel_philox(const ChannelArgs &c, void *stream) {
    if (c.frames <= 0) return FPLDPC_OK;
    const PhiloxArgs a = args(c, c.n);
    const uint64_t threads = (uint64_t)c.frames * (((uint64_t)c.n + 1) / 2);
    const uint64_t blocks = (threads + kChanThreads - 1) / kChanThreads;
    if (blocks > 0x7fffffffull) return fail(FPLDPC_ERR_ARG, "channel: too many values for one call (frames * n)");
    hipLaunchKernelGGL(philox_channel_kernel, dim3((unsigned)blocks), dim3(kChanThreads), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : hip_fail(e, "philox channel kernel launch");
}

int launch_bias_patch_philox(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, const ChannelArgs &c,
                             void *stream) {
    if (c.frames <= 0 || (b.count() == 0 && !c.logw)) return FPLDPC_OK;
    PhiloxArgs a = args(c, b.n);
    a.count = b.count();
    a.pos = d_pos;
    a.shift = d_shift;
    a.logw = c.logw;
    hipLaunchKernelGGL(philox_patch_kernel, dim3((unsigned)((c.frames + kPer - 1) / kPer)), dim3(kPatchThreads), 0,
                       (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : hip_fail(e, "philox patch kernel launch");
}

}  // namespace fpldpc

using namespace fpldpc;

extern "C" {

int fpldpc_channel_llr_src(int32_t source, int64_t seed, int64_t first_frame, int32_t frames, int32_t n, double snr,
                           double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out,
                           int32_t out_type, int32_t *overflow, void *stream) {
    if (source == FPLDPC_NOISE_LEHMER)
        return fpldpc_channel_llr(seed, first_frame, frames, n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type,
                                  overflow, stream);
    if (source != FPLDPC_NOISE_PHILOX) return bad_source();
    const ChannelArgs a{seed, first_frame, frames, n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, overflow};
    if (const int st = philox_rules(a)) return st;
    return launch_channel_philox(a, stream);
}

int fpldpc_bias_channel_llr_src(fpldpc_bias_t b, int32_t source, int64_t seed, int64_t first_frame, int32_t frames,
                                double snr, double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame,
                                void *out, int32_t out_type, int32_t *overflow, double *logw, void *stream) {
    if (source == FPLDPC_NOISE_LEHMER)
        return fpldpc_bias_channel_llr(b, seed, first_frame, frames, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type,
                                       overflow, logw, stream);
    if (source != FPLDPC_NOISE_PHILOX) return bad_source();
    if (!b) return fail(FPLDPC_ERR_ARG, "bias: null bias");
    const ChannelArgs a{seed, first_frame, frames, b->n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, overflow, logw};
    if (const int st = philox_rules(a)) return st;
    if (frames == 0) return FPLDPC_OK;
    if (const int st = bias_bind(b)) return st;
    if (const int st = launch_channel_philox(a, stream)) return st;
    return launch_bias_patch_philox(*b, b->d_pos, b->d_shift, a, stream);
}

}  // extern "C"
