// uastc_rdo_strips.h -- how uastc_rdo cuts a slice into strips, and rdo_slices_layout: the strip table and THE statement of the device workspace of every RDO call,
// over one slice (bu_hip_k_uastc_rdo, a pipeline submission) or several (bu_hip_k_uastc_rdo_slices). Plain host code: api_uastc.cpp builds the layout before anything
// is enqueued, the launchers of uastc_rdo_kernels.hip read it, and tests/test_uastc_rdo_slices_host.py builds it into a stand-alone program.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace bu {

// one slice: uastc_rdo, uastc_enc.cpp:4103-4111. per_job 0 = one strip; hist_cap = entries of a strip's selector history
inline void rdo_strip_layout(uint32_t n, uint32_t total_jobs, uint32_t& per_job, uint32_t& n_strips, uint32_t& hist_cap) {
    per_job = total_jobs ? n / total_jobs : 0;
    if (total_jobs <= 1 || per_job <= 8) { per_job = 0; n_strips = 1; }
    else n_strips = (n + per_job - 1) / per_job;
    const uint32_t longest = per_job ? per_job : n;
    hist_cap = 64;
    while (hist_cap < 4 * (uint64_t)longest && hist_cap < (1u << 30)) hist_cap <<= 1;  // load <= 1/4: a bucket of 4 holds one key on average
}

// What the kernels read of a strip. first / last / mod_ofs are indices into the concatenated arrays of the call, hist_ofs counts history entries.
struct rdo_strip_rec { uint32_t first, last, hist_cap, mod_ofs; uint64_t hist_ofs; uint32_t slice, pad; };

constexpr size_t RDO_INFO_BYTES = 32, RDO_HIST_ENTRY_BYTES = 16, RDO_TABLE_BYTES = 2048;   // per block, per history entry, per block (uastc_rdo_kernels.hip asserts them)
constexpr uint32_t RDO_SLICES_MAX_BLOCKS = 0x7FFFFFFFu;   // the walk holds block indices in signed ints

struct rdo_slices_layout {
    std::vector<rdo_strip_rec> recs;      // in block order: a block finds its strip by bisecting `first`. A slice of 0 blocks has no record.
    std::vector<uint32_t> order;          // workgroup w of a walk takes recs[order[w]]: non-increasing strip length, ties in block order
    std::vector<uint32_t> slice_strips;   // per slice, what uastc_rdo_strips() says of it alone (1 for an empty slice)
    uint32_t n_slices = 0, total_blocks = 0, longest = 0;   // longest: blocks of the longest strip = the longest mod_list a strip can have
    // byte offsets into the workspace; [0, zero_bytes) is cleared before the prepare pass
    size_t counters = 0, strip_counts = 0, strip_flags = 0, hist = 0, state = 0, zero_bytes = 0, strips = 0, order_at = 0, info = 0, mod_list = 0, table = 0, total_bytes = 0;
};

// false: the block total does not fit (RDO_SLICES_MAX_BLOCKS)
inline bool rdo_slices_layout_build(const uint32_t* slice_blocks, uint32_t n_slices, uint32_t total_jobs, rdo_slices_layout& L) {
    L = rdo_slices_layout();
    L.n_slices = n_slices;
    uint64_t at = 0, hist_at = 0;
    for (uint32_t s = 0; s < n_slices; s++) {
        const uint32_t n = slice_blocks[s];
        if (at + n > RDO_SLICES_MAX_BLOCKS) return false;
        uint32_t per_job, n_strips, cap;
        rdo_strip_layout(n, total_jobs, per_job, n_strips, cap);
        L.slice_strips.push_back(n_strips);
        for (uint32_t k = 0; n && k < n_strips; k++) {
            rdo_strip_rec r;
            r.first = (uint32_t)at + (per_job ? k * per_job : 0u);
            r.last = per_job ? (uint32_t)at + std::min(n, (k + 1) * per_job) : (uint32_t)at + n;
            r.hist_cap = cap; r.mod_ofs = r.first; r.hist_ofs = hist_at; r.slice = s; r.pad = 0;
            hist_at += cap;
            L.longest = std::max(L.longest, r.last - r.first);
            L.recs.push_back(r);
        }
        at += n;
    }
    L.total_blocks = (uint32_t)at;
    const uint32_t S = (uint32_t)L.recs.size();
    L.order.resize(S);
    for (uint32_t i = 0; i < S; i++) L.order[i] = i;
    std::stable_sort(L.order.begin(), L.order.end(), [&](uint32_t a, uint32_t b) { return L.recs[a].last - L.recs[a].first > L.recs[b].last - L.recs[b].first; });
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    L.counters = o; o += up((size_t)n_slices * 16);   // per slice: modified, failed, refined, skipped
    L.strip_counts = o; o += up((size_t)S * 4);
    L.strip_flags = o; o += up((size_t)S * 4);
    L.hist = o; o += up((size_t)hist_at * RDO_HIST_ENTRY_BYTES);
    L.state = o; o += up(L.total_blocks);
    L.zero_bytes = o;
    L.strips = o; o += up((size_t)S * sizeof(rdo_strip_rec));
    L.order_at = o; o += up((size_t)S * 4);
    L.info = o; o += up((size_t)L.total_blocks * RDO_INFO_BYTES);
    L.mod_list = o; o += up((size_t)L.total_blocks * 4);
    L.table = o; o += up((size_t)L.total_blocks * RDO_TABLE_BYTES);
    L.total_bytes = o;
    return true;
}

// One slice alone. Its records are what the arithmetic form of the kernels computes from a strip's index (first = k * per_job, hist_ofs = k * hist_cap, one hist_cap),
// so that form runs on this layout without the table on the device: the strips / order_at regions then lie unused.
inline bool rdo_slice_layout_build(uint32_t n, uint32_t total_jobs, rdo_slices_layout& L) { return rdo_slices_layout_build(&n, 1, total_jobs, L); }
// what bu_hip_k_uastc_rdo needs for n blocks; 0: more blocks than a call takes
inline size_t uastc_rdo_workspace_bytes(uint32_t n, uint32_t total_jobs) {
    rdo_slices_layout L;
    return rdo_slice_layout_build(n, total_jobs, L) ? L.total_bytes : 0;
}

} // namespace bu
