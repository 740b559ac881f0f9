// fpldpc_channel.cpp -- the reference harness's channel model on the host: Lehmer uniforms with
// O(log k) skip-ahead, Odeh-Evans normals, BPSK/AWGN LLR quantisation.  Frames are independent
// given the skip-ahead, so generation is split over threads by frame range.  Beside it the host twins of the
// counter-based noise source (FPLDPC_NOISE_PHILOX, include/fpldpc.h; the kernels are fpldpc_source.hip's) and the
// *_src_host entry points that take a source.  One frame loop (channel_host) serves them all: a noise source gives
// it the normal variate of each position, and a bias, where there is one, its shifted positions.
//
// Reference: Random() rngs.cpp:52-69 (m = 2^31-1, a = 48271, Schrage), Normal() rvgs.cpp:152-181,
// LLR quantisation PerfTest.cpp:108-120 / 168-169 / 287-297.
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "fpldpc_bias.hpp"
#include "fpldpc_channel_args.hpp"
#include "fpldpc_internal.hpp"
#include "fpldpc_source.hpp"

// Bit parity with the gcc/glibc-built reference needs the exact operation sequence: no FMA
// contraction of the Odeh-Evans polynomials or the LLR scaling.
#pragma clang fp contract(off)

using fpldpc::ChannelArgs;

namespace {

constexpr int64_t kModulus = 2147483647;  // rngs.cpp:40
constexpr int64_t kMultiplier = 48271;    // rngs.cpp:41

inline double lehmer_next(int64_t *state) {
    const int64_t Q = kModulus / kMultiplier, R = kModulus % kMultiplier;
    const int64_t s = *state;
    const int64_t t = kMultiplier * (s % Q) - R * (s / Q);
    *state = t > 0 ? t : t + kModulus;
    return (double)*state / kModulus;
}

inline double odeh_evans_normal(int64_t *state, double sigma) {
    const double p0 = 0.322232431088, q0 = 0.099348462606;
    const double p1 = 1.0, q1 = 0.588581570495;
    const double p2 = 0.342242088547, q2 = 0.531103462366;
    const double p3 = 0.204231210245e-1, q3 = 0.103537752850;
    const double p4 = 0.453642210148e-4, q4 = 0.385607006340e-2;
    const double u = lehmer_next(state);
    const double t = u < 0.5 ? sqrt(-2.0 * log(u)) : sqrt(-2.0 * log(1.0 - u));
    const double p = p0 + t * (p1 + t * (p2 + t * (p3 + t * p4)));
    const double q = q0 + t * (q1 + t * (q2 + t * (q3 + t * q4)));
    const double z = u < 0.5 ? (p / q) - t : t - (p / q);
    return 0.0 + sigma * z;  // Normal(m = 0, s = sigma)
}

inline int64_t mulmod(int64_t a, int64_t b) { return (int64_t)(((__int128)a * b) % kModulus); }

// A noise source of channel_host: made once per thread for the frames from f_lo on, then asked for the normal
// variate of every position of every frame, in order.
// The Lehmer stream: one skip-ahead to the range's first draw, then Odeh-Evans variates drawn in order.
struct LehmerSource {
    int64_t state;
    double sigma;
    LehmerSource(const ChannelArgs &a, int64_t f_lo)
        : state(fpldpc_rng_skip(a.seed, (uint64_t)(a.first_frame + f_lo) * (uint64_t)a.n)), sigma(a.sigma) {}
    double normal(int64_t, int) { return odeh_evans_normal(&state, sigma); }
};

// FPLDPC_NOISE_PHILOX (include/fpldpc.h): one call per pair gives its two variates, rad * (cos, sin)(2 pi u2); every
// value is a pure function of (seed, frame, position), so neither the split nor the call's frame range changes one.
struct PhiloxSource {
    uint64_t seed, first_frame;
    double sigma, z[2] = {0.0, 0.0};
    PhiloxSource(const ChannelArgs &a, int64_t)
        : seed((uint64_t)a.seed), first_frame((uint64_t)a.first_frame), sigma(a.sigma) {}
    double normal(int64_t f, int i) {
        if (!(i & 1)) {
            double u1, u2;
            fpldpc::philox_uniforms(seed, first_frame + (uint64_t)f, (uint32_t)i >> 1, &u1, &u2);
            const double rad = sqrt(-2.0 * log(u1));
            const double ang = (2.0 * M_PI) * u2;
            z[0] = rad * cos(ang);
            z[1] = rad * sin(ang);
        }
        return 0.0 + sigma * z[i & 1];
    }
};

// The channel over a.frames frames on host threads, after the entry point's argument checks.  b may be null (the
// plain channel).  With one, the mean is shifted on its positions and each frame's log-weight is summed over them in
// ascending j: the host twin of the patch kernels (fpldpc_bias.hip, fpldpc_source.hip).
template <typename Source>
int channel_host(const ChannelArgs &a, const fpldpc_bias *b, int nthreads) {
    if (a.frames == 0) return FPLDPC_OK;
    const int n = a.n, count = b ? b->count() : 0;
    const double snr = a.snr, sigma = a.sigma;
    unsigned hw = std::thread::hardware_concurrency();
    int T = nthreads > 0 ? nthreads : (int)(hw ? hw : 1);
    T = std::max(1, std::min(T, a.frames));
    std::vector<int> overflow(T, 0);
    auto work = [&](int t) {
        const int64_t f_lo = (int64_t)a.frames * t / T, f_hi = (int64_t)a.frames * (t + 1) / T;
        Source src(a, f_lo);
        const double scale = (double)(1 << a.frac_bits);
        for (int64_t f = f_lo; f < f_hi; f++) {
            const uint8_t *c = a.cw ? a.cw + (a.cw_per_frame ? (size_t)f * n : 0) : nullptr;
            double sum = 0.0;
            int j = 0;
            for (int i = 0; i < n; i++) {
                const int s = 1 - 2 * (c ? (int)(c[i] & 1) : 0);
                const double nrm = src.normal(f, i);
                double llr;
                if (j < count && b->pos[j] == i) {
                    const double sh = b->shift[j++];
                    llr = (2 * snr) * (s * (1 - sh) + nrm);
                    sum = sum + sh * (2 * s * nrm - sh) / (2 * sigma * sigma);
                } else {
                    llr = 2 * snr * (s + nrm);
                }
                const size_t at = (size_t)f * n + i;
                if (a.out_type == FPLDPC_LLR_F64) {
                    static_cast<double *>(a.out)[at] = llr;
                    continue;
                }
                const int32_t q = (int32_t)(llr * scale);  // int() truncation, no clipping
                if (a.out_type == FPLDPC_LLR_I32) {
                    static_cast<int32_t *>(a.out)[at] = q;
                } else {
                    if (q < -32768 || q > 32767) overflow[t] = 1;
                    static_cast<int16_t *>(a.out)[at] = (int16_t)q;
                }
            }
            if (a.logw) a.logw[f] = sum;
        }
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < T; t++)
        if (overflow[t]) return fpldpc::fail(FPLDPC_ERR_ARG, "LLR does not fit int16");
    return FPLDPC_OK;
}

int philox_channel_host(const fpldpc_bias *b, const ChannelArgs &a, int32_t nthreads) {
    if (const int st = fpldpc::philox_rules(a)) return st;
    return channel_host<PhiloxSource>(a, b, nthreads);
}

int bad_source() { return fpldpc::fail(FPLDPC_ERR_ARG, "bad noise source (FPLDPC_NOISE_LEHMER or FPLDPC_NOISE_PHILOX)"); }

}  // namespace

extern "C" {

int64_t fpldpc_rng_skip(int64_t seed, uint64_t draws) {
    int64_t r = 1, b = kMultiplier;
    while (draws) {
        if (draws & 1) r = mulmod(r, b);
        b = mulmod(b, b);
        draws >>= 1;
    }
    return mulmod(seed, r);
}

int fpldpc_channel_llr_host(int64_t seed, int64_t first_frame, int32_t frames, int32_t n, double snr,
                            double sigma, int32_t frac_bits, const uint8_t *cw, void *out, int32_t out_type,
                            int32_t nthreads) {
    if (!out || frames < 0 || n <= 0 || first_frame < 0 || frac_bits < 0 || frac_bits > 24 || seed <= 0 ||
        seed >= kModulus)
        return fpldpc::fail(FPLDPC_ERR_ARG, "bad channel arguments");
    if (out_type != FPLDPC_LLR_I32 && out_type != FPLDPC_LLR_I16 && out_type != FPLDPC_LLR_F64)
        return fpldpc::fail(FPLDPC_ERR_ARG, "bad out_type");
    return channel_host<LehmerSource>({seed, first_frame, frames, n, snr, sigma, frac_bits, cw, 0, out, out_type}, nullptr,
                                      nthreads);
}

// The host twin of fpldpc_bias_channel_llr (fpldpc_bias.hip)
int fpldpc_bias_channel_llr_host(fpldpc_bias_t b, int64_t seed, int64_t first_frame, int32_t frames, double snr, double sigma,
                                 int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out, int32_t out_type,
                                 double *logw, int32_t nthreads) {
    if (!b) return fpldpc::fail(FPLDPC_ERR_ARG, "bias: null bias");
    if (!out || frames < 0 || first_frame < 0 || frac_bits < 0 || frac_bits > 24 || seed <= 0 || seed >= kModulus)
        return fpldpc::fail(FPLDPC_ERR_ARG, "bias: bad channel arguments");
    if (out_type != FPLDPC_LLR_I32 && out_type != FPLDPC_LLR_I16 && out_type != FPLDPC_LLR_F64)
        return fpldpc::fail(FPLDPC_ERR_ARG, "bias: bad out_type");
    if (cw_per_frame != 0 && cw_per_frame != 1) return fpldpc::fail(FPLDPC_ERR_ARG, "bias: cw_per_frame must be 0 or 1");
    return channel_host<LehmerSource>(
        {seed, first_frame, frames, b->n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, nullptr, logw}, b, nthreads);
}

void fpldpc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    fpldpc::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

int fpldpc_channel_llr_src_host(int32_t source, int64_t seed, int64_t first_frame, int32_t frames, int32_t n, double snr,
                                double sigma, int32_t frac_bits, const uint8_t *cw, void *out, int32_t out_type,
                                int32_t nthreads) {
    if (source == FPLDPC_NOISE_LEHMER)
        return fpldpc_channel_llr_host(seed, first_frame, frames, n, snr, sigma, frac_bits, cw, out, out_type, nthreads);
    if (source != FPLDPC_NOISE_PHILOX) return bad_source();
    return philox_channel_host(nullptr, {seed, first_frame, frames, n, snr, sigma, frac_bits, cw, 0, out, out_type}, nthreads);
}

int fpldpc_bias_channel_llr_src_host(fpldpc_bias_t b, int32_t source, int64_t seed, int64_t first_frame, int32_t frames,
                                     double snr, double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame,
                                     void *out, int32_t out_type, double *logw, int32_t nthreads) {
    if (source == FPLDPC_NOISE_LEHMER)
        return fpldpc_bias_channel_llr_host(b, seed, first_frame, frames, snr, sigma, frac_bits, cw, cw_per_frame, out,
                                            out_type, logw, nthreads);
    if (source != FPLDPC_NOISE_PHILOX) return bad_source();
    if (!b) return fpldpc::fail(FPLDPC_ERR_ARG, "bias: null bias");
    return philox_channel_host(
        b, {seed, first_frame, frames, b->n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, nullptr, logw}, nthreads);
}

}  // extern "C"
