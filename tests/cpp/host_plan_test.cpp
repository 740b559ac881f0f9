// host_plan_test.cpp -- CPU check of the decoders' host staging layout, slot-major index table and packed
// reference mask (fixedpointldpc_amd/csrc/fpldpc_host_plan.hpp) against their definitions restated here.
//
// Staging layout: for random (batch, n, element sizes, wanted outputs) the LLRs and every wanted output have a
// 256-byte aligned region of at least their raw size inside the block, no two regions overlap, and an output
// not wanted has none; with every output wanted and 2- or 4-byte LLRs the offsets are those of the layout the
// fixed-point decoders' host decode has always used (every region padded to 256 bytes, in the order llr, hard,
// iters, syndrome flags, post, bit errors, totals).
// Table: against a double loop over (check, slot) for random irregular codes, at pitch m and at m rounded up to
// 64, in the code's own order and in a stable sort by degree, for two fill values.
// Mask: random distinct position sets on n = 31, 32, 33, 169 and 2209 (positions 0, 31, 32 and n - 1 always
// among them, bits any byte) against a loop over the variables; one position repeated gives the empty result.
// Exit 0 = all trials agree.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "fpldpc_host_plan.hpp"

using namespace fpldpc::plan;

namespace {

struct Region {
    size_t at, raw;
};

int check_layout(std::mt19937_64 &rng) {
    static const size_t kElem[] = {2, 4, 8};
    const size_t batch = 1 + rng() % 5000, n = 1 + rng() % 3000;
    const size_t llr_elem = kElem[rng() % 3], post_elem = kElem[1 + rng() % 2];
    const unsigned want = (unsigned)(rng() % 64);
    const StageLayout l = stage_layout(batch, n, llr_elem, post_elem, want);
    const size_t hw = (n + 31) / 32;
    const size_t off[7] = {l.llr, l.hard, l.iters, l.syn_ok, l.post, l.bit_errors, l.totals};
    const size_t raw[7] = {batch * n * llr_elem, batch * hw * 4, batch * 4, batch, batch * n * post_elem, batch * 4, 32};
    int bad = 0;
    std::vector<Region> rs;
    for (int i = 0; i < 7; ++i) {
        const bool wanted = i == 0 || (want >> (i - 1) & 1);
        if (!wanted) {
            bad += off[i] != kNoRegion;
            continue;
        }
        if (off[i] == kNoRegion || off[i] % 256 != 0 || off[i] + raw[i] > l.bytes) {
            ++bad;
            continue;
        }
        rs.push_back({off[i], raw[i]});
    }
    for (size_t i = 0; i < rs.size(); ++i)
        for (size_t j = 0; j < i; ++j) bad += rs[i].at < rs[j].at + rs[j].raw && rs[j].at < rs[i].at + rs[i].raw;
    if (want == kAllOutputs && llr_elem != 8) {
        // the fixed-point host decode's layout, as it stood before the layout became a function
        auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t llr_b = align(batch * n * llr_elem), hard_b = align(batch * hw * 4), it_b = align(batch * 4),
                     ok_b = align(batch), post_b = align(batch * n * 4), be_b = align(batch * 4), tot_b = align(32);
        const StageLayout f = stage_layout(batch, n, llr_elem, 4, want);
        size_t p = 0;
        bad += f.llr != p;
        p += llr_b;
        bad += f.hard != p;
        p += hard_b;
        bad += f.iters != p;
        p += it_b;
        bad += f.syn_ok != p;
        p += ok_b;
        bad += f.post != p;
        p += post_b;
        bad += f.bit_errors != p;
        p += be_b;
        bad += f.totals != p;
        bad += f.bytes != p + tot_b;
    }
    if (bad) fprintf(stderr, "layout: batch %zu n %zu elems %zu/%zu want %u\n", batch, n, llr_elem, post_elem, want);
    return bad;
}

int check_table(std::mt19937_64 &rng) {
    const int m = 1 + (int)(rng() % 200), dc_max = 2 + (int)(rng() % 30), n = dc_max + (int)(rng() % 5000);
    std::vector<int32_t> cdeg(m), clist((size_t)m * dc_max, -1);
    for (int r = 0; r < m; ++r) {
        cdeg[r] = r == 0 ? dc_max : 1 + (int)(rng() % dc_max);
        for (int k = 0; k < cdeg[r]; ++k) clist[(size_t)r * dc_max + k] = (int32_t)(rng() % n);
    }
    std::vector<int> identity(m), sorted(m);
    for (int r = 0; r < m; ++r) identity[r] = sorted[r] = r;
    std::stable_sort(sorted.begin(), sorted.end(), [&](int x, int y) { return cdeg[x] < cdeg[y]; });
    int bad = 0;
    for (int form = 0; form < 6; ++form) {
        const size_t pitch = form & 1 ? ((size_t)m + 63) / 64 * 64 : (size_t)m;
        const int *order = form < 2 ? nullptr : form < 4 ? identity.data() : sorted.data();
        const int rows = dc_max + (form & 1 ? (int)(rng() % 4) : 0);  // a kernel's DC may exceed dc_max
        const uint16_t fill = form & 1 ? 0 : 0xffff;
        const SlotTable t = slot_table(m, dc_max, cdeg.data(), clist.data(), rows, pitch, order, fill);
        if (t.vidx.size() != (size_t)rows * pitch || t.cdeg.size() != (size_t)m) {
            ++bad;
            continue;
        }
        for (int k = 0; k < rows; ++k)
            for (size_t j = 0; j < pitch; ++j) {
                uint16_t want = fill;
                if (j < (size_t)m) {
                    const int r = form < 4 ? (int)j : sorted[j];
                    if (k < cdeg[r]) want = (uint16_t)clist[(size_t)r * dc_max + k];
                }
                bad += t.vidx[(size_t)k * pitch + j] != want;
            }
        for (int j = 0; j < m; ++j) bad += t.cdeg[j] != (uint8_t)cdeg[form < 4 ? j : sorted[j]];
    }
    if (bad) fprintf(stderr, "table: m %d dc_max %d\n", m, dc_max);
    return bad;
}

// A set of k distinct positions of n (every one with full: k = n) holding 0, 31, 32 and n - 1 where they exist,
// in random order, with bytes as bits: the mask against a loop over the variables; then the same list with each
// of its positions in turn repeated at a random place, which must give the empty result.
int check_mask(std::mt19937_64 &rng, int n, bool full) {
    std::vector<int32_t> pos(n);
    for (int v = 0; v < n; ++v) pos[v] = v;
    std::shuffle(pos.begin(), pos.end(), rng);
    const int32_t edge[4] = {0, 31, 32, n - 1};
    int front = 0;
    for (int32_t e : edge)
        if (e < n && std::find(pos.begin(), pos.begin() + front, e) == pos.begin() + front)
            std::iter_swap(std::find(pos.begin(), pos.end(), e), pos.begin() + front++);
    const int k = full ? n : front + (int)(rng() % (n - front + 1));
    pos.resize(k);
    std::shuffle(pos.begin(), pos.end(), rng);
    std::vector<uint8_t> bits(k);
    for (auto &b : bits) b = (uint8_t)rng();  // any byte: only bit 0 counts
    const size_t hw = ((size_t)n + 31) / 32;
    std::vector<int> is_info(hw * 32, 0), ref(hw * 32, 0);
    for (int i = 0; i < k; ++i) {
        is_info[pos[i]] = 1;
        ref[pos[i]] = bits[i] & 1;
    }
    const std::vector<uint32_t> mk = reference_mask(n, pos.data(), bits.data(), k);
    int bad = mk.size() != 2 * hw;
    for (size_t v = 0; !bad && v < hw * 32; ++v) {
        bad += (int)(mk[v / 32] >> (v % 32) & 1) != is_info[v];
        bad += (int)(mk[hw + v / 32] >> (v % 32) & 1) != ref[v];
    }
    for (int i = 0; i < k; ++i) {
        std::vector<int32_t> p2 = pos;
        std::vector<uint8_t> b2 = bits;
        const size_t at = rng() % (k + 1);
        p2.insert(p2.begin() + at, pos[i]);
        b2.insert(b2.begin() + at, (uint8_t)rng());
        bad += !reference_mask(n, p2.data(), b2.data(), k + 1).empty();
    }
    if (bad) fprintf(stderr, "mask: n %d k %d\n", n, k);
    return bad;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261021);
    int bad = 0, trials = 0;
    for (int t = 0; t < 20000; ++t, ++trials) bad += check_layout(rng) != 0;
    for (int t = 0; t < 300; ++t, ++trials) bad += check_table(rng) != 0;
    for (int n : {31, 32, 33, 169, 2209})
        for (int t = 0; t < 8; ++t, ++trials) bad += check_mask(rng, n, t == 0) != 0;
    printf("%d trials, %d mismatches\n", trials, bad);
    return bad != 0;
}
