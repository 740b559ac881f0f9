// fpldpc_minsum_wide.hip -- gfx950 (CDNA4) "wide" form of the two min-sum decoders: check degrees up to 255
// (DESIGN.md "Min-sum decoders: check degrees above 64").  flood_minsum_choose and layered_minsum_choose
// (fpldpc_minsum.hip, fpldpc_layered_minsum.hip) hand every code with dc_max > 64, and every code under
// FPLDPC_MINSUM_FORM=wide, to minsum_wide_choose / minsum_wide_launch below.
//
// Nothing of the definitions changes: the schedules are those of flood_minsum and layered_minsum, the frame
// framework is fpldpc_layered_device.hpp's, the check rule is fpldpc_minsum_device.hpp's.  What differs:
//
//   * The slot loops are run-time loops over the check's degree, 32 slots -- one sign word -- at a time; the 32
//     slots of a chunk are unrolled, so a chunk's gathers are all in flight at once.  The degree predicates
//     eight slots at a time (a group wholly past it is skipped); inside a group a slot past the degree reads
//     the check's last slot again and is neutralised arithmetically (32 lane masks held across the loops
//     spill scalar registers).
//   * A lane cannot hold a value per slot, so each pass walks the index table: pass 1 gathers, rebuilds the old
//     messages and tracks m1, m2, k1 and the sign bits; pass 2 walks the slots again and emits new[k] (flooding:
//     the atomic add into `nxt`; layered: t[k] recomputed from the posterior, which only this lane writes and
//     has not written yet, and the old sign word, which is read before the new one replaces it).
//   * The check state is W = ceil(dc_max / 32) sign words beside the two magnitudes and k1, 8 + 4 W bytes per
//     check, kept word-major: word i of check c at state[i * m + c] (consecutive lanes on consecutive words),
//         word 0 = f(m1) | f(m2) << 16;  word 1 = k1 | parity of the sign bits << 31;  word 2 + w = sign bits
//         of slots 32 w .. 32 w + 31 (bit k & 31 = s[k]).
//     An all-zero entry rebuilds every message to 0.  The new sign words of a check (at most 8) stay in
//     registers between the passes, selected by compare chains, never by a run-time register index.
//   * Table addressing only (a forward array code gets its index table built), always a degree table.
//
// LDS, state in LDS (both: the index table [dc_max][m] uint16 and then the degree table [m] uint8 follow):
//     flooding: state [2 + W][m] uint32 | acc [3][n] int32 | llr [n] int16 (to a word) | misc [kLayMisc]
//     layered:  post [n] int16 (to a word) | misc [kLayMisc] | state [2 + W][m] uint32
// "global": LDS is the int16 vector, the control words and the degree table where it fits; the state (and the
// flooding accumulators behind it) is slice blockIdx.x of the decoder's scratch, rounded up to 256 bytes.  The
// memory ordering is that of fpldpc_minsum_global.hip: a slice belongs to one workgroup, state words are plain
// accesses ordered by barriers (and touched by one lane only), the flooding accumulators change by atomics that
// return nothing and are read by relaxed agent-scope atomic loads.
#include "fpldpc_layered_host.hpp"
#include "fpldpc_minsum_device.hpp"

namespace fpldpc {
namespace {

struct WideArgs {
    LayeredArgs a;  // as the other min-sum kernels read it (vidx always set)
    int scale_16 = 16, offset = 0;
    int W = 3;      // sign words per check
};

constexpr int kWideMaxDeg = 255;   // the degree tables are uint8
constexpr int kWideMaxWords = 8;   // ceil(255 / 32)

__host__ __device__ constexpr size_t wd_state_bytes(int m, int W) { return (size_t)(2 + W) * m * sizeof(uint32_t); }
__host__ __device__ constexpr size_t wd_vec_words(int n) { return ((size_t)n * sizeof(int16_t) + 3) / 4; }
// state in LDS: bytes before the index table
__host__ __device__ constexpr size_t wd_flood_llr_offset(int n, int m, int W) { return wd_state_bytes(m, W) + 3 * sizeof(int) * (size_t)n; }
__host__ __device__ constexpr size_t wd_flood_table_offset(int n, int m, int W) {
    return wd_flood_llr_offset(n, m, W) + (wd_vec_words(n) + kLayMisc) * sizeof(int);
}
__host__ __device__ constexpr size_t wd_layered_table_offset(int n, int m, int W) {
    return (wd_vec_words(n) + kLayMisc) * sizeof(int) + wd_state_bytes(m, W);
}
// state global: LDS bytes before the degree table, and the slices
__host__ __device__ constexpr size_t wd_global_base(int n) { return (wd_vec_words(n) + kLayMisc) * sizeof(int); }
__host__ __device__ constexpr bool wd_deg_in_lds(int n, int m) { return wd_global_base(n) + (size_t)m <= kLdsMax; }
__host__ __device__ constexpr size_t wd_round_slice(size_t bytes) { return (bytes + 255) / 256 * 256; }
__host__ __device__ constexpr size_t wd_flood_slice(int n, int m, int W) {
    return wd_round_slice(wd_state_bytes(m, W) + 3 * sizeof(int) * (size_t)n);
}
__host__ __device__ constexpr size_t wd_layered_slice(int m, int W) { return wd_round_slice(wd_state_bytes(m, W)); }

// The index table and the degree table behind `tail` in LDS (state in LDS), or the degree table alone behind
// the control words where it fits (state global).  (The first frame pull's barriers come before the first read.)
__device__ __forceinline__ void wd_tables(const LayeredArgs &a, char *tail, bool lds_state, const uint16_t **vidx,
                                          const uint8_t **cdeg) {
    *vidx = a.vidx;
    *cdeg = a.cdeg;
    if (lds_state && a.table_lds) {
        const int edges = a.dc_max * a.m;
        uint16_t *const lv = reinterpret_cast<uint16_t *>(tail);
        for (int i = threadIdx.x; i < edges; i += blockDim.x) lv[i] = a.vidx[i];
        *vidx = lv;
        tail += (size_t)edges * sizeof(uint16_t);
    }
    if (lds_state || wd_deg_in_lds(a.n, a.m)) {
        uint8_t *const ld = reinterpret_cast<uint8_t *>(tail);
        for (int i = threadIdx.x; i < a.m; i += blockDim.x) ld[i] = a.cdeg[i];
        *cdeg = ld;
    }
}

// 1 if some check is unsatisfied by hard[v] = neg(v) (workgroup-uniform; a barrier).  The degree is the check's
// own, at run time; four reads in flight.
template <typename Neg>
__device__ __forceinline__ int wd_syndrome(int m, const uint16_t *vidx, const uint8_t *cdeg, Neg neg) {
    int fail = 0;
    for (int c = threadIdx.x; c < m; c += blockDim.x) {
        const int deg = cdeg[c];
        const uint16_t *tab = vidx + c;
        int par = 0;
#pragma unroll 4
        for (int k = 0; k < deg; ++k) par ^= neg((int)tab[(size_t)k * m]);
        fail |= par;
    }
    return __syncthreads_or(fail);
}

// A check's messages from its two magnitudes, k1 and one sign word already flipped by the check's parity
// (bit i: message k = k0 + i is negative).
__device__ __forceinline__ int wd_message(int M1, int M2, int k1, uint32_t flipped, int k, int i) {
    return ms_signed(k == k1 ? M2 : M1, (int)(flipped << (31 - i)) >> 31);
}

// The stored part of a check that the slots share: magnitudes, k1 and the parity as a 0 / ~0 word.
struct WdHead {
    int M1, M2, k1;
    uint32_t flip;
    __device__ __forceinline__ WdHead(uint32_t w0, uint32_t w1)
        : M1((int)(w0 & 0xffff)), M2((int)(w0 >> 16)), k1((int)(w1 & 0xff)), flip(0u - (w1 >> 31)) {}
};

// Pass 1 of check c (column `tab` = vidx + c, state column `st` = state + c): gathers with get(v), rebuilds the
// old messages and tracks the minima, k1 and the sign words (nw[w], in registers).  Stores the words 0 and 1 of
// the new entry -- the caller holds the old ones in `old` -- and returns the new head; the sign words are
// stored by pass 2, which may still need the old ones.
template <typename Get>
__device__ __forceinline__ WdHead wd_pass1(const uint16_t *tab, uint32_t *st, int m, int deg, const WdHead &old, int Sm,
                                           const WideArgs &wa, uint32_t (&nw)[kWideMaxWords], Get get) {
    int m1 = 0x7fff, m2 = 0x7fff, k1 = 0;
    uint32_t all = 0;
#pragma unroll
    for (int j = 0; j < kWideMaxWords; ++j) nw[j] = 0;
    for (int w = 0, k0 = 0; k0 < deg; ++w, k0 += 32) {
        const uint16_t *col = tab + (size_t)k0 * m;
        // gather: the chunk's reads in flight at once
        const int left = deg - k0;  // slots of the check in this chunk and after it (>= 1)
        int x[32];
#pragma unroll
        for (int g = 0; g < 32; g += 8) {
#pragma unroll
            for (int i = g; i < g + 8; ++i) x[i] = 0;
            if (g >= left) continue;
#pragma unroll
            for (int i = g; i < g + 8; ++i) x[i] = get((int)col[(size_t)min(i, left - 1) * m]);
        }
        const uint32_t ow = st[(size_t)(2 + w) * m] ^ old.flip;
        uint32_t s = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if ((i & ~7) >= left) continue;
            const int t = lay_clamp(x[i] - wd_message(old.M1, old.M2, old.k1, ow, k0 + i, i), Sm);
            // a slot past the degree: magnitude 0x7fff changes neither minimum nor k1, its sign bit is masked below
            const int mag = max(t, -t) | (((left - 1 - i) >> 31) & 0x7fff);
            s |= ((uint32_t)(t - 1) >> 31) << i;  // t <= 0
            m2 = min(m2, max(mag, m1));
            k1 = mag < m1 ? k0 + i : k1;
            m1 = min(m1, mag);
        }
        s &= left >= 32 ? ~0u : (1u << left) - 1;
#pragma unroll
        for (int j = 0; j < kWideMaxWords; ++j) nw[j] = j == w ? s : nw[j];
        all ^= s;
    }
    const uint32_t w0 = (uint32_t)ms_correct(m1, wa.scale_16, wa.offset) | (uint32_t)ms_correct(m2, wa.scale_16, wa.offset) << 16;
    const uint32_t w1 = (uint32_t)k1 | (uint32_t)(__popc(all) & 1) << 31;
    st[0] = w0;
    st[m] = w1;
    return WdHead(w0, w1);
}

__device__ __forceinline__ uint32_t wd_word(const uint32_t (&nw)[kWideMaxWords], int w) {
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < kWideMaxWords; ++j) s = j == w ? nw[j] : s;
    return s;
}

template <bool GLOBAL>
__device__ __forceinline__ int wd_acc_load(const int *p) {
    if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}

// The flooding schedule of flood_minsum (one lane per check over all m checks, three rotating int32
// accumulators, integer atomics into `nxt`, one barrier, the syndrome).  GLOBAL: state and accumulators in
// the workgroup's slice.
template <bool GLOBAL>
__global__ void __launch_bounds__(kLayMaxNT) flood_minsum_wide(WideArgs wa) {
    const LayeredArgs &a = wa.a;
    extern __shared__ __attribute__((aligned(16))) int wd_smem[];
    const int n = a.n, m = a.m, W = wa.W;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    char *const smem = reinterpret_cast<char *>(wd_smem);
    char *const home = GLOBAL ? static_cast<char *>(a.c2v_scratch) + (size_t)blockIdx.x * wd_flood_slice(n, m, W) : smem;
    uint32_t *const state = reinterpret_cast<uint32_t *>(home);
    int *const acc = reinterpret_cast<int *>(home + wd_state_bytes(m, W));
    int16_t *const llr = reinterpret_cast<int16_t *>(GLOBAL ? smem : smem + wd_flood_llr_offset(n, m, W));
    int *const misc = reinterpret_cast<int *>(llr) + wd_vec_words(n);
    const uint16_t *vidx;
    const uint8_t *cdeg;
    wd_tables(a, reinterpret_cast<char *>(misc + kLayMisc), !GLOBAL, &vidx, &cdeg);

    for (;;) {
        const int cw = lay_next_frame(a, misc);
        if (cw < 0) break;
        // offsets into acc of the three accumulators: step 1 reads L from `cur` and adds into `nxt`
        int cur = 0, nxt = n, spare = 2 * n;
        for (int v = tid; v < n; v += NT) {
            const int x = lay_clamp(lay_load_llr(a, (size_t)cw * n + v), Sp);
            llr[v] = (int16_t)x;
            acc[cur + v] = x;
            acc[nxt + v] = x;
        }
        for (int i = tid; i < (2 + W) * m; i += NT) state[i] = 0;  // every c2v = 0
        __syncthreads();
        // the channel pre-check, as the other min-sum kernels: 0 iterations, posteriors left untouched
        if (a.precheck && !wd_syndrome(m, vidx, cdeg, [&](int v) { return llr[v] <= 0; })) {
            lay_store(a, cw, llr, false, 0, 1, misc);
            continue;
        }
        int iters = 0, fail = 1;
        for (int it = 1; it <= a.max_iter; ++it) {
            // the accumulator of step it + 1 starts at L (idle in this step: last read before the syndrome barrier)
            for (int v = tid; v < n; v += NT) acc[spare + v] = llr[v];
            for (int c = tid; c < m; c += NT) {
                const int deg = cdeg[c];
                const uint16_t *const tab = vidx + c;
                uint32_t *const st = state + c;
                const WdHead old(st[0], st[m]);
                uint32_t nw[kWideMaxWords];
                const int *const from = acc + cur;
                const WdHead nh = wd_pass1(tab, st, m, deg, old, Sm, wa, nw, [&](int v) { return lay_clamp(wd_acc_load<GLOBAL>(from + v), Sp); });
                // pass 2: new[k] into the next step's accumulator
                int *const to = acc + nxt;
                for (int w = 0, k0 = 0; k0 < deg; ++w, k0 += 32) {
                    const uint16_t *col = tab + (size_t)k0 * m;
                    const uint32_t s = wd_word(nw, w);
                    st[(size_t)(2 + w) * m] = s;
                    const int left = deg - k0;
                    int v[32];
#pragma unroll
                    for (int g = 0; g < 32; g += 8) {
#pragma unroll
                        for (int i = g; i < g + 8; ++i) v[i] = 0;
                        if (g >= left) continue;
#pragma unroll
                        for (int i = g; i < g + 8; ++i) v[i] = col[(size_t)min(i, left - 1) * m];
                    }
                    // eight slots under one predicate; inside, a slot past the degree adds 0 to the last slot's variable
#pragma unroll
                    for (int g = 0; g < 32; g += 8) {
                        if (g >= left) continue;
#pragma unroll
                        for (int i = g; i < g + 8; ++i)
                            atomicAdd(&to[v[i]], wd_message(nh.M1, nh.M2, nh.k1, s ^ nh.flip, k0 + i, i) & ~((left - 1 - i) >> 31));
                    }
                }
            }
            __syncthreads();  // every message of the step is in `nxt`
            const int *const sum = acc + nxt;  // the raw sum has the posterior's sign
            fail = wd_syndrome(m, vidx, cdeg, [&](int v) { return wd_acc_load<GLOBAL>(sum + v) <= 0; });
            iters = it;
            if ((a.early_term && !fail) || it == a.max_iter) break;
            const int done = cur;
            cur = nxt;
            nxt = spare;
            spare = done;
        }
        // the frame's posteriors: the last step's accumulator, clamped in place
        for (int v = tid; v < n; v += NT) acc[nxt + v] = lay_clamp(wd_acc_load<GLOBAL>(&acc[nxt + v]), Sp);
        __syncthreads();
        lay_store(a, cw, acc + nxt, true, iters, !fail, misc);
    }
    lay_leave(a);
}

// The layered schedule of layered_minsum (lane j on check l*L + j, int16 posteriors in LDS, one barrier between
// layers).  GLOBAL: the state in the workgroup's slice.
template <bool GLOBAL>
__global__ void __launch_bounds__(kLayMaxNT) layered_minsum_wide(WideArgs wa) {
    const LayeredArgs &a = wa.a;
    extern __shared__ __attribute__((aligned(16))) int wd_smem[];
    const int n = a.n, m = a.m, W = wa.W;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    int16_t *const post = reinterpret_cast<int16_t *>(wd_smem);
    int *const misc = wd_smem + wd_vec_words(n);
    uint32_t *const lds_state = reinterpret_cast<uint32_t *>(misc + kLayMisc);
    uint32_t *const state = GLOBAL ? reinterpret_cast<uint32_t *>(static_cast<char *>(a.c2v_scratch) + (size_t)blockIdx.x * wd_layered_slice(m, W))
                                   : lds_state;
    const uint16_t *vidx;
    const uint8_t *cdeg;
    wd_tables(a, reinterpret_cast<char *>(GLOBAL ? lds_state : lds_state + (size_t)(2 + W) * m), !GLOBAL, &vidx, &cdeg);

    for (;;) {
        const int cw = lay_next_frame(a, misc);
        if (cw < 0) break;
        for (int v = tid; v < n; v += NT) post[v] = (int16_t)lay_clamp(lay_load_llr(a, (size_t)cw * n + v), Sp);
        for (int i = tid; i < (2 + W) * m; i += NT) state[i] = 0;  // every c2v = 0
        __syncthreads();
        // the channel pre-check, as the other layered kernels: 0 iterations, posteriors left untouched
        if (a.precheck && !wd_syndrome(m, vidx, cdeg, [&](int v) { return post[v] <= 0; })) {
            lay_store(a, cw, post, false, 0, 1, misc);
            continue;
        }
        int iters = 0, fail = 1;
        for (int it = 1; it <= a.max_iter; ++it) {
            for (int l = 0; l < a.layers; ++l) {
                for (int j = tid; j < a.L; j += NT) {
                    const int c = l * a.L + j;
                    const int deg = cdeg[c];
                    const uint16_t *const tab = vidx + c;
                    uint32_t *const st = state + c;
                    const WdHead old(st[0], st[m]);
                    uint32_t nw[kWideMaxWords];
                    const WdHead nh = wd_pass1(tab, st, m, deg, old, Sm, wa, nw, [&](int v) { return (int)post[v]; });
                    // pass 2: t[k] again from the posterior still there and the old entry, then the new posterior
                    for (int w = 0, k0 = 0; k0 < deg; ++w, k0 += 32) {
                        const uint16_t *col = tab + (size_t)k0 * m;
                        const uint32_t ow = st[(size_t)(2 + w) * m] ^ old.flip;
                        const uint32_t s = wd_word(nw, w);
                        st[(size_t)(2 + w) * m] = s;
                        const int left = deg - k0;
                        uint32_t pk[32];  // v_k << 16 | (uint16) post[v_k]
#pragma unroll
                        for (int g = 0; g < 32; g += 8) {
#pragma unroll
                            for (int i = g; i < g + 8; ++i) pk[i] = 0;
                            if (g >= left) continue;
#pragma unroll
                            for (int i = g; i < g + 8; ++i) {
                                const uint32_t v = col[(size_t)min(i, left - 1) * m];
                                pk[i] = v << 16 | (uint16_t)post[v];
                            }
                        }
                        // no predicate: a slot past the degree is the check's last slot once more, in index and in
                        // sign bit, and stores that slot's value to that slot's variable again
#pragma unroll
                        for (int i = 0; i < 32; ++i) {
                            if ((i & ~7) >= left) continue;
                            const int e = min(i, left - 1);
                            const int t = lay_clamp((int)(int16_t)(pk[i] & 0xffffu) - wd_message(old.M1, old.M2, old.k1, ow, k0 + e, e), Sm);
                            post[pk[i] >> 16] = (int16_t)lay_clamp(t + wd_message(nh.M1, nh.M2, nh.k1, s ^ nh.flip, k0 + e, e), Sp);
                        }
                    }
                }
                __syncthreads();  // the next layer reads the posteriors this one wrote
            }
            fail = wd_syndrome(m, vidx, cdeg, [&](int v) { return post[v] <= 0; });
            iters = it;
            if (a.early_term && !fail) break;
        }
        lay_store(a, cw, post, true, iters, !fail, misc);
    }
    lay_leave(a);
}

using WideFn = void (*)(WideArgs);
WideFn wide_fn(const LayeredChoice &lc) {
    if (lc.mode == kFloodMinsum) return lc.lds_state ? flood_minsum_wide<false> : flood_minsum_wide<true>;
    return lc.lds_state ? layered_minsum_wide<false> : layered_minsum_wide<true>;
}

int wide_words(const LayeredChoice &lc) { return lc.dc / 32; }

}  // namespace

bool minsum_form_forced_wide() {
    const char *s = getenv("FPLDPC_MINSUM_FORM");
    return s && !strcmp(s, "wide");
}

// Envelope: check degrees 2..255 and n <= 65535.  The state in LDS wherever the bytes before the index table
// (and one byte per check of the degree table) fit the CU's 160 KiB, unless force_global; there the index table
// is placed under `table_env` as in the other forms.  Otherwise the global form: the table global, one slice
// per resident workgroup.
int minsum_wide_choose(const fpldpc_code &code, int mode, int threads, const char *table_env, bool force_global, int device,
                       LayeredChoice *out) {
    const bool flood = mode == kFloodMinsum;
    const char *who = flood ? "flooding min-sum" : "layered min-sum";
    for (int r = 0; r < code.m; r++)
        if (code.cdeg[r] < 2) return fail(FPLDPC_ERR_UNSUPPORTED, "check of degree < 2 (reference behaviour undefined)");
    if (code.dc_max > kWideMaxDeg) return fail(FPLDPC_ERR_UNSUPPORTED, std::string(who) + " decoder: check degree above 255");
    if (code.n > 65535) return fail(FPLDPC_ERR_UNSUPPORTED, std::string(who) + " decoder: more than 65535 variables");
    LayeredChoice lc;
    const int W = (code.dc_max + 31) / 32;
    lc.mode = mode;
    lc.wide = true;
    lc.dc = 32 * W;
    lc.state_bytes = (int)((2 + W) * sizeof(uint32_t));
    lc.threads = threads;
    const char *kernel = flood ? "flood_minsum_wide" : "layered_minsum_wide";
    const size_t base = (flood ? wd_flood_table_offset(code.n, code.m, W) : wd_layered_table_offset(code.n, code.m, W)) + (size_t)code.m;
    if (base > kLdsMax || force_global) {
        lc.lds_bytes = wd_global_base(code.n) + (wd_deg_in_lds(code.n, code.m) ? (size_t)code.m : 0);
        LayResidency<WideFn> resident{wide_fn(lc), lc.threads};
        const int per_cu = resident(lc.lds_bytes);
        if (int st = lay_grid(per_cu, resident.e, device, who, &lc.grid)) return st;
        lc.scratch_bytes = (size_t)lc.grid * (flood ? wd_flood_slice(code.n, code.m, W) : wd_layered_slice(code.m, W));
        snprintf(lc.name, sizeof lc.name, "%s<DC=%d,addr=gtable,deg=table,mem=global>", kernel, lc.dc);
    } else {
        lc.lds_state = true;
        if (int st = lay_choose_lds(wide_fn(lc), code, base, table_env, device, who, kernel, &lc)) return st;
    }
    *out = lc;
    return FPLDPC_OK;
}

int minsum_wide_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    return lay_launch(wide_fn(lc), lc, args, WideArgs{args, scale_16, offset, wide_words(lc)}, stream,
                      lc.mode == kFloodMinsum ? "flooding min-sum" : "layered min-sum");
}

}  // namespace fpldpc
