// fpldpc_bias.hip -- mean-shift importance sampling on chosen positions (include/fpldpc.h, fpldpc_bias_t): the
// bias object, its device tables, and the patch kernel that turns the LLRs of a channel call into those of the
// shifted channel and gives every frame its log-weight.  This unit is outside the kernel build id, as the
// harvest, layered, min-sum and simulation-source units are.
//
// For a biased position i = pos[j] of frame f, with s = 1 - 2c[i], z the Odeh-Evans variate of draw f*n + i and
// nrm = 0.0 + sigma*z exactly as channel_kernel forms them (fpldpc_gen.hip):
//     LLR     = (2*snr) * (s*(1 - a[j]) + nrm)                 each operation rounded once, no contraction
//     LLR_fp  = (int)(LLR * 2^frac_bits)
//     term_j  = a[j] * (2*s*nrm - a[j]) / (2*sigma*sigma)
//     logw[f] = sum_j term_j
// w = exp(logw[f]) is the ratio of the true density N(s, sigma^2) to the shifted density N(s(1 - a), sigma^2) at
// the received values.  Two things a user of the weight must know:
//   - The reference's variates come from a 31-bit uniform (Random() rngs.cpp:52-69), so |z| is bounded near 6.2:
//     the weight is exact for the Gaussian that the stream approximates, not for its truncation.
//   - One call carries one bias.  Mixing several biases, and multiplying by the size of a structure's orbit under
//     the code's automorphisms, is the caller's arithmetic.
//
// Launch order: launch_channel, then, on the same stream, bias_patch_kernel over the same output.  A wave per
// frame, kPer frames per workgroup.  Lane l takes the biased positions j = l, l + 64, ...: it jumps to draw
// f*n + pos[j] by the a^(2^k) table, forms z and nrm, overwrites the LLR at pos[j] in the output type, corrects
// *overflow by (new value outside int16) - (old value outside int16) -- the old value recomputed from the same
// nrm, as the stored one is truncated -- with an integer atomic only where that difference is not zero, and adds
// term_j to its own sum in ascending j.  The 64 lane sums are then reduced by an xor butterfly (__shfl_xor, strides
// 32 .. 1), a fixed order, and lane 0 stores logw[f]: no floating-point atomic, so a call made twice gives the same
// bits.  No LDS, no scratch.
//
// The Lehmer step, the skip-ahead and the Odeh-Evans variate below are a second copy of channel_kernel's
// (fpldpc_gen.hip): moving them into a header that both units include changed two instructions of channel_kernel
// (a loop guard's compare polarity and the operand order of one multiply), and with them the kernel build id, so
// fpldpc_gen.hip stays as it is.  tests/test_gpu_bias_channel.py holds the two copies together: a zero shift must
// reproduce the channel's output bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>

#include "fpldpc_bias.hpp"
#include "fpldpc_internal.hpp"

namespace fpldpc {
namespace {

constexpr uint64_t kMod = 2147483647ull;  // rngs.cpp:40
constexpr uint64_t kMul = 48271ull;       // rngs.cpp:41
constexpr int kPowBits = 48;              // draw indices < 2^48, as the channel
constexpr int kWave = 64;
constexpr int kPer = 8;                   // frames per workgroup
constexpr int kThreads = kWave * kPer;

struct BiasArgs {
    uint64_t apow[kPowBits];  // a^(2^j) mod m
    uint64_t seed;
    int64_t first_frame;
    int frames, n, frac, out_type, cw_per_frame, count;
    double snr, sigma;
    const uint8_t *cw;
    const int32_t *pos;
    const double *shift;
    void *out;
    int *overflow;
    double *logw;
};

__device__ __forceinline__ uint64_t mulmod(uint64_t x, uint64_t y) {  // x, y < 2^31
    const uint64_t p = x * y;                                          // < 2^62
    uint64_t r = (p & kMod) + (p >> 31);                               // Mersenne fold
    r = (r & kMod) + (r >> 31);
    return r >= kMod ? r - kMod : r;
}

__global__ void __launch_bounds__(kThreads) bias_patch_kernel(BiasArgs a) {
    const int lane = threadIdx.x % kWave;
    const int64_t f = (int64_t)blockIdx.x * kPer + threadIdx.x / kWave;
    if (f >= a.frames) return;  // the whole wave
    const double scale = (double)(1 << a.frac);
    const uint8_t *cw = a.cw ? a.cw + (a.cw_per_frame ? (size_t)f * a.n : 0) : nullptr;
    const size_t base = (size_t)f * a.n;
    const uint64_t frame_draw = (uint64_t)(a.first_frame + f) * (uint64_t)a.n;
    const double two_snr = __dmul_rn(2.0, a.snr);
    const double den = __dmul_rn(__dmul_rn(2.0, a.sigma), a.sigma);
    double sum = 0.0;
    int ovf = 0;
    for (int j = lane; j < a.count; j += kWave) {
        const int i = a.pos[j];
        const double sh = a.shift[j];
        // state after D draws = seed * a^D: the next Random() returns draw D + 1's state
        uint64_t D = frame_draw + (uint64_t)i;
        uint64_t s = a.seed;
#pragma unroll 1
        for (int k = 0; D; ++k, D >>= 1)
            if (D & 1) s = mulmod(s, a.apow[k]);
        s = mulmod(s, kMul);  // Random()
        const double u = (double)s / (double)kMod;
        // Normal(0, sigma): Odeh & Evans (rvgs.cpp:159-180), the operations of channel_kernel
        const double p0 = 0.322232431088, q0 = 0.099348462606;
        const double p1 = 1.0, q1 = 0.588581570495;
        const double p2 = 0.342242088547, q2 = 0.531103462366;
        const double p3 = 0.204231210245e-1, q3 = 0.103537752850;
        const double p4 = 0.453642210148e-4, q4 = 0.385607006340e-2;
        const double t = u < 0.5 ? sqrt(-2.0 * log(u)) : sqrt(-2.0 * log(1.0 - u));
        const double p = __dadd_rn(p0, __dmul_rn(t, __dadd_rn(p1, __dmul_rn(t, __dadd_rn(p2, __dmul_rn(t, __dadd_rn(p3, __dmul_rn(t, p4))))))));
        const double q = __dadd_rn(q0, __dmul_rn(t, __dadd_rn(q1, __dmul_rn(t, __dadd_rn(q2, __dmul_rn(t, __dadd_rn(q3, __dmul_rn(t, q4))))))));
        const double z = u < 0.5 ? __dsub_rn(__ddiv_rn(p, q), t) : __dsub_rn(t, __ddiv_rn(p, q));
        const double nrm = __dadd_rn(0.0, __dmul_rn(a.sigma, z));
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

// the existing channel's own argument rules (fpldpc_channel_llr), n the bias's
int channel_rules(const fpldpc_bias *b, int64_t seed, int64_t first_frame, int32_t frames, int32_t frac_bits, const void *out,
                  int32_t out_type, int32_t cw_per_frame) {
    if (!b) return fail(FPLDPC_ERR_ARG, "bias: null bias");
    if (!out || frames < 0 || first_frame < 0 || frac_bits < 0 || frac_bits > 24 || seed <= 0 || seed >= 2147483647 ||
        (uint64_t)(first_frame + frames) * (uint64_t)b->n >= (1ull << kPowBits))
        return fail(FPLDPC_ERR_ARG, "bias: bad channel arguments");
    if (out_type != FPLDPC_LLR_I32 && out_type != FPLDPC_LLR_I16 && out_type != FPLDPC_LLR_F64)
        return fail(FPLDPC_ERR_ARG, "bias: bad out_type");
    if (cw_per_frame != 0 && cw_per_frame != 1) return fail(FPLDPC_ERR_ARG, "bias: cw_per_frame must be 0 or 1");
    return FPLDPC_OK;
}

}  // namespace

int bias_upload_tables(const fpldpc_bias &b, int32_t **d_pos, double **d_shift) {
    *d_pos = nullptr;
    *d_shift = nullptr;
    const size_t c = b.pos.size();
    if (!c) return FPLDPC_OK;
    hipError_t e = hipMalloc((void **)d_pos, c * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)d_shift, c * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(*d_pos, b.pos.data(), c * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*d_shift, b.shift.data(), c * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(*d_pos);
        (void)hipFree(*d_shift);
        *d_pos = nullptr;
        *d_shift = nullptr;
        return hip_fail(e, "bias tables (hipMalloc / hipMemcpy)");
    }
    return FPLDPC_OK;
}

int bias_bind(fpldpc_bias *b) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (b->device >= 0 && b->device != dev) return fail(FPLDPC_ERR_ARG, "bias already bound to another device");
    if (b->device < 0) {
        if (const int st = bias_upload_tables(*b, &b->d_pos, &b->d_shift)) return st;
        b->device = dev;
    }
    return FPLDPC_OK;
}

int launch_bias_patch(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, const ChannelArgs &c, void *stream) {
    if (c.frames <= 0 || (b.count() == 0 && !c.logw)) return FPLDPC_OK;
    BiasArgs a;
    uint64_t x = kMul;
    for (int j = 0; j < kPowBits; ++j) {
        a.apow[j] = x;
        x = (uint64_t)(((unsigned __int128)x * x) % kMod);
    }
    a.seed = (uint64_t)c.seed;
    a.first_frame = c.first_frame;
    a.frames = c.frames;
    a.n = b.n;
    a.frac = c.frac_bits;
    a.out_type = c.out_type;
    a.cw_per_frame = c.cw_per_frame;
    a.count = b.count();
    a.snr = c.snr;
    a.sigma = c.sigma;
    a.cw = c.cw;
    a.pos = d_pos;
    a.shift = d_shift;
    a.out = c.out;
    a.overflow = c.overflow;
    a.logw = c.logw;
    hipLaunchKernelGGL(bias_patch_kernel, dim3((unsigned)((c.frames + kPer - 1) / kPer)), dim3(kThreads), 0, (hipStream_t)stream,
                       a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FPLDPC_OK : hip_fail(e, "bias patch kernel launch");
}

}  // namespace fpldpc

using namespace fpldpc;

fpldpc_bias::~fpldpc_bias() {
    if (d_pos) (void)hipFree(d_pos);
    if (d_shift) (void)hipFree(d_shift);
}

extern "C" {

int fpldpc_bias_create(int32_t n, const int32_t *pos, const double *shift, int32_t count, fpldpc_bias_t *out) {
    if (!out) return fail(FPLDPC_ERR_ARG, "bias: null argument");
    if (n <= 0) return fail(FPLDPC_ERR_ARG, "bias: n must be positive");
    if (count < 0 || count > n) return fail(FPLDPC_ERR_ARG, "bias: count must be in 0 .. n");
    if (count > 0 && (!pos || !shift)) return fail(FPLDPC_ERR_ARG, "bias: null argument");
    for (int j = 0; j < count; ++j) {
        if (pos[j] < 0 || pos[j] >= n) return fail(FPLDPC_ERR_ARG, "bias: position out of range (0 <= pos < n)");
        if (j && pos[j] <= pos[j - 1])
            return fail(FPLDPC_ERR_ARG, "bias: positions must be strictly ascending (unsorted or duplicate)");
        if (!std::isfinite(shift[j])) return fail(FPLDPC_ERR_ARG, "bias: shift must be finite");
    }
    std::unique_ptr<fpldpc_bias> b(new fpldpc_bias());
    b->n = n;
    b->pos.assign(pos, pos + count);
    b->shift.assign(shift, shift + count);
    *out = b.release();
    return FPLDPC_OK;
}

void fpldpc_bias_free(fpldpc_bias_t b) { delete b; }

int fpldpc_bias_dims(fpldpc_bias_t b, int32_t dims[2]) {
    if (!b || !dims) return fail(FPLDPC_ERR_ARG, "bias: null argument");
    dims[0] = b->n;
    dims[1] = b->count();
    return FPLDPC_OK;
}

int fpldpc_bias_sums_get(fpldpc_bias_t b, fpldpc_bias_sums *out) {
    if (!b || !out) return fail(FPLDPC_ERR_ARG, "bias: null argument");
    *out = b->sums;
    return FPLDPC_OK;
}

int fpldpc_bias_channel_llr(fpldpc_bias_t b, int64_t seed, int64_t first_frame, int32_t frames, double snr, double sigma,
                            int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out, int32_t out_type,
                            int32_t *overflow, double *logw, void *stream) {
    if (const int st = channel_rules(b, seed, first_frame, frames, frac_bits, out, out_type, cw_per_frame)) return st;
    if (frames == 0) return FPLDPC_OK;
    if (const int st = bias_bind(b)) return st;
    if (const int st = launch_channel(seed, first_frame, frames, b->n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type,
                                      overflow, stream))
        return st;
    const ChannelArgs a{seed, first_frame, frames, b->n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, overflow, logw};
    return launch_bias_patch(*b, b->d_pos, b->d_shift, a, stream);
}

}  // extern "C"
