// fpldpc_host_plan.hpp -- the layout of a decoder's host staging block, the slot-major index table of a
// code and the packed reference mask, as the decoders' host code (fpldpc_host.cpp, fpldpc_layered.cpp,
// fpldpc_decoder.cpp) uses them.  Header-only, no HIP: the CPU test tests/cpp/host_plan_test.cpp checks
// each against its definition restated there.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fpldpc {
namespace plan {

// The optional outputs of a decode call, as bits of `want`.
enum : unsigned { kHard = 1, kIters = 2, kSynOk = 4, kPost = 8, kBitErrors = 16, kTotals = 32, kAllOutputs = 63 };
constexpr size_t kStageAlign = 256;
constexpr size_t kNoRegion = ~(size_t)0;

// Byte offsets into one device block: the LLRs [batch][n] of llr_elem bytes first, then every wanted
// output in the order of the bits above, each region 256-byte aligned and padded; kNoRegion for an output
// not wanted (it takes no room).  hard is [batch][ceil(n / 32)] words, iters and bit_errors int32
// [batch], syn_ok a byte per frame, post [batch][n] of post_elem bytes, totals four int64.
struct StageLayout {
    size_t llr = 0, hard = kNoRegion, iters = kNoRegion, syn_ok = kNoRegion, post = kNoRegion, bit_errors = kNoRegion,
           totals = kNoRegion;
    size_t bytes = 0;
};

inline StageLayout stage_layout(size_t batch, size_t n, size_t llr_elem, size_t post_elem, unsigned want) {
    StageLayout l;
    auto take = [&l](size_t raw) {
        const size_t at = l.bytes;
        l.bytes += (raw + kStageAlign - 1) & ~(kStageAlign - 1);
        return at;
    };
    l.llr = take(batch * n * llr_elem);
    if (want & kHard) l.hard = take(batch * ((n + 31) / 32) * 4);
    if (want & kIters) l.iters = take(batch * 4);
    if (want & kSynOk) l.syn_ok = take(batch);
    if (want & kPost) l.post = take(batch * n * post_elem);
    if (want & kBitErrors) l.bit_errors = take(batch * 4);
    if (want & kTotals) l.totals = take(32);
    return l;
}

// Slot-major index table of a code in alist form (cdeg [m], clist [m][dc_max], clist order = fold order):
// vidx[k * pitch + j] = clist[order[j]][k] for k < cdeg[order[j]], `fill` in every other entry of the
// rows * pitch (rows >= dc_max, pitch >= m), and cdeg[j] = cdeg[order[j]] as bytes.  order null: the
// code's own check order.
struct SlotTable {
    std::vector<uint16_t> vidx;
    std::vector<uint8_t> cdeg;
};

inline SlotTable slot_table(int m, int dc_max, const int32_t *cdeg, const int32_t *clist, int rows, size_t pitch,
                            const int *order, uint16_t fill) {
    SlotTable t;
    t.vidx.assign((size_t)rows * pitch, fill);
    t.cdeg.resize(m);
    for (int j = 0; j < m; j++) {
        const int r = order ? order[j] : j;
        t.cdeg[j] = (uint8_t)cdeg[r];
        for (int k = 0; k < cdeg[r]; k++) t.vidx[(size_t)k * pitch + j] = (uint16_t)clist[(size_t)r * dc_max + k];
    }
    return t;
}

// The reference bits of k positions in a code of n variables as [2][ceil(n / 32)] words, the form the packed
// kernels count bit errors from their hard-decision words with: bit v of the first half is set for every
// position v, bit v of the second half is bit 0 of that position's reference bit.  Empty when a position
// repeats (the index form counts such a position once per occurrence; a mask cannot).
inline std::vector<uint32_t> reference_mask(int n, const int32_t *info_index, const uint8_t *info_bits, int k) {
    const size_t hw = ((size_t)n + 31) / 32;
    std::vector<uint32_t> mk(2 * hw, 0);
    for (int i = 0; i < k; i++) {
        const int v = info_index[i];
        if (mk[v / 32] >> (v % 32) & 1) return {};
        mk[v / 32] |= 1u << (v % 32);
        mk[hw + v / 32] |= (uint32_t)(info_bits[i] & 1) << (v % 32);
    }
    return mk;
}

}  // namespace plan
}  // namespace fpldpc
