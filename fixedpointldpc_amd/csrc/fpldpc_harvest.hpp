// fpldpc_harvest.hpp -- the harvest object (fpldpc_harvest_t) and what fpldpc_sim.cpp takes from
// fpldpc_harvest.hip: the check table of the scan kernel and the launchers of the scan and of the ordered
// compaction of a chunk's codeword-error frames.
#pragma once
#include <cstdint>
#include <atomic>
#include <unordered_map>
#include <vector>

#include "fpldpc_internal.hpp"

// One harvest: the code's check lists (copied at creation), the device table of the public scan (bound on
// first use), and the records, counts and classes of the last simulation.
struct fpldpc_harvest {
    int n = 0, m = 0, dc = 0;
    int hard_words = 0, syn_words = 0;
    int max_records = 0;
    std::vector<int32_t> clist;  // [m][dc], -1 padded, as fpldpc_code keeps it
    int device = -1;             // fpldpc_harvest_scan: the device d_table lives on
    uint16_t *d_table = nullptr;
    // results
    int64_t counts[6] = {0, 0, 0, 0, 0, 0};  // frames, codeword_errors, detected, undetected, recorded, dropped
    std::vector<int64_t> frame;
    std::vector<int32_t> iters, info_errors, weight, unsat;
    std::vector<uint32_t> err;  // [recorded][hard_words]
    std::vector<uint32_t> syn;  // [recorded][syn_words]
    std::unordered_map<uint64_t, int64_t> classes;  // weight << 32 | unsat -> frames (sorted when reported)
    // max_records records are held: a simulation's later chunks need no rows (set by the appending thread,
    // read by every rank's when it submits a chunk)
    std::atomic<bool> full{false};
    ~fpldpc_harvest();
    void clear();
    // one counted frame, in frame order; row = its err words then its syn words (read only for a record)
    void add_frame(int64_t f, int32_t its, int32_t blk, int32_t w, int32_t u, const uint32_t *row) {
        ++counts[0];
        if (w > 0) add_error_frame(f, its, blk, w, u, row);
    }
    void add_error_frame(int64_t f, int32_t its, int32_t blk, int32_t w, int32_t u, const uint32_t *row);
};

namespace fpldpc {

constexpr uint16_t kHarvestPad = 0xffff;  // a table slot past a check's degree (variables are < 65535)

// The scan's check table on the current device: uint16 [dc][m], slot k of check c at k * m + c, so that a
// wave's lanes (a check each) read consecutive entries.  The caller frees *out with hipFree.
int harvest_upload_table(const fpldpc_harvest &h, uint16_t **out);

// weight / unsat / err / syn of `batch` frames (include/fpldpc.h, fpldpc_harvest_scan); table on the
// stream's device.  err / syn rows have pitch err_pitch / syn_pitch words (>= hard_words / syn_words).
int launch_harvest_scan(const fpldpc_harvest &h, const uint16_t *table, const uint32_t *hard, const uint8_t *cw,
                        int cw_per_frame, int batch, int32_t *weight, int32_t *unsat, uint32_t *err, int err_pitch,
                        uint32_t *syn, int syn_pitch, void *stream);

// Ordered compaction: rows [batch][row_words] of the frames with weight > 0, in frame order, to
// rec [cap][row_words]; frames beyond the first `cap` such frames are left out.  pos [batch] is scratch.
int launch_harvest_compact(const int32_t *weight, const uint32_t *rows, int row_words, int batch, int cap, int32_t *pos,
                           uint32_t *rec, void *stream);

}  // namespace fpldpc
