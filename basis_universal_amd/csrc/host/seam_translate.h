// seam_translate.h -- the host translations of section 1 of include/basisu_hip.h (the reference's encoder/basisu_opencl.h layouts) into the forms the
// device-resident layer takes. No HIP in here: api_etc1s.cpp calls these and does the copies and launches; tests/native/seam_translate_host.cpp compiles
// them for the CPU-only suite (tests/test_seam_translate_host.py).
//
// Every function validates BEFORE it writes: it returns nullptr and fills `out`, or returns a static error text and leaves `out` as it was. Nothing
// reads past what the caller's counts cover, so a bad caller gets 0 from the entry point and never an out-of-bounds read, on the host or the device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "../../../include/basisu_hip.h"

namespace bu {
namespace seam {

constexpr uint32_t MAX_WINDOWS = 255;                    // the device layer's block -> parent table is one byte per block
constexpr uint64_t MAX_EXPANDED_TEXELS = 0x7FFFFFFFull;  // pixel clusters, whole call: what the kernels' 32-bit texel arithmetic addresses

// ---- etc_block packing (basisu_etc.h:91-103: a big-endian u64; the returned value is in MEMORY order, memcpy it)

inline uint64_t be64(uint64_t v) { return __builtin_bswap64(v); }

// ETC1S block of colour5 + intensity table: differential mode with zero deltas, both table fields = inten, diff and flip bits set, selectors zero
inline uint64_t color5_inten_to_etc_block(uint32_t r5, uint32_t g5, uint32_t b5, uint32_t inten) {
    return be64(((uint64_t)r5 << 59) | ((uint64_t)g5 << 51) | ((uint64_t)b5 << 43) | ((uint64_t)inten << 37) | ((uint64_t)inten << 34) | (3ull << 32));
}

// fosc_selector_struct's 2-bit selectors, texel p = y * 4 + x at bits [2p, 2p + 2) (frontend.cpp:2462-2464) -> the selector bytes of an etc_block:
// raw ETC selector = 0x4B >> 2s (selector 0..3 -> 3, 2, 0, 1), its low bit at bit x * 4 + y of the low plane, its high bit 16 above (etc.h:232-236)
inline uint64_t selectors_to_etc_block(uint32_t packed) {
    uint32_t bits = 0;
    for (uint32_t p = 0; p < 16; p++) {
        const uint32_t s = (packed >> (p * 2)) & 3u, x = p & 3u, y = p >> 2;
        const uint32_t raw = (0x4Bu >> (s * 2)) & 3u, bit = x * 4 + y;
        bits |= ((raw & 1u) << bit) | ((raw >> 1) << (16 + bit));
    }
    return be64((uint64_t)bits);
}

// ---- candidate windows -> parent lists

// One "parent" per DISTINCT (first, count) window, in order of first use; its list is the positions first .. first + count - 1 of the flat array.
// Windows may overlap, nest or share a first offset. A window a block uses must be non-empty and lie inside the flat array.
struct windows {
    std::vector<uint32_t> cand_offsets, cand_indices;   // CSR over positions in the flat array: n_parents + 1 offsets
    std::vector<uint8_t> block_parent;                  // per block
    uint32_t n_parents() const { return (uint32_t)cand_offsets.size() - 1; }
};

// get_window(b, first, count) reads block b's window
template <typename F>
inline const char* build_windows(uint32_t n_blocks, uint64_t flat_entries, F get_window, windows& out, const char* past_end, const char* empty, const char* too_many) {
    windows w;
    w.cand_offsets.assign(1, 0);
    w.block_parent.resize(n_blocks);
    std::unordered_map<uint64_t, uint32_t> parent_of;   // (first, count) -> parent
    uint64_t last_key = ~0ull; uint32_t last_parent = 0;   // runs of blocks share a window
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint32_t f, c;
        get_window(b, f, c);
        if ((uint64_t)f + c > flat_entries) return past_end;
        if (!c) return empty;
        const uint64_t key = ((uint64_t)f << 32) | c;
        if (key != last_key) {
            auto it = parent_of.find(key);
            if (it == parent_of.end()) {
                if (parent_of.size() == MAX_WINDOWS) return too_many;
                it = parent_of.emplace(key, (uint32_t)parent_of.size()).first;
                for (uint32_t k = 0; k < c; k++) w.cand_indices.push_back(f + k);
                w.cand_offsets.push_back((uint32_t)w.cand_indices.size());
            }
            last_key = key; last_parent = it->second;
        }
        w.block_parent[b] = (uint8_t)last_parent;
    }
    out = std::move(w);
    return nullptr;
}

// ---- refine_endpoint_clusterization (cl_block_info_struct / cl_endpoint_cluster_struct, frontend.cpp:1684-1750)

struct refine_tables {
    std::vector<uint32_t> params;      // per POSITION of the flat array: r5 | g5 << 8 | b5 << 16 | inten << 24
    windows win;
    std::vector<uint32_t> block_cur;   // per block: the position, inside its window, of the entry whose m_cluster_index is the block's current cluster
};

inline const char* translate_refine(const bu_block_info* info, uint32_t n_blocks, uint32_t total_clusters, const bu_endpoint_cluster* clusters, refine_tables& out) {
    if ((n_blocks && !info) || (total_clusters && !clusters)) return "refine: null pointer";
    refine_tables t;
    if (const char* e = build_windows(n_blocks, total_clusters, [&](uint32_t b, uint32_t& f, uint32_t& c) { f = info[b].m_first_cluster_ofs; c = info[b].m_num_clusters; }, t.win,
                                      "refine: candidate window past the end of the cluster list", "refine: empty candidate window",
                                      "refine: more than 255 distinct candidate windows"))
        return e;
    // The kernel's pruning threshold, its intensity filter (frontend.cpp:1811-1815) and its tie rule all go by the block's current cluster, which the
    // reference always files in the block's own window (frontend.cpp:971-996): a block whose current cluster is elsewhere is refused, not guessed at.
    // One look-up table per parent, filled on first use: (cluster index << 32 | position) ascending, so the first position of an index comes first.
    t.block_cur.resize(n_blocks);
    std::vector<std::vector<uint64_t>> pos_of(t.win.n_parents());
    for (uint32_t b = 0; b < n_blocks; b++) {
        const uint32_t p = t.win.block_parent[b], f = info[b].m_first_cluster_ofs, c = info[b].m_num_clusters;
        std::vector<uint64_t>& tab = pos_of[p];
        if (tab.empty()) {
            tab.resize(c);
            for (uint32_t k = 0; k < c; k++) tab[k] = ((uint64_t)clusters[f + k].m_cluster_index << 32) | (f + k);
            std::sort(tab.begin(), tab.end());
        }
        const uint64_t want = (uint64_t)info[b].m_cur_cluster_index << 32;
        const auto it = std::lower_bound(tab.begin(), tab.end(), want);
        if (it == tab.end() || (*it >> 32) != info[b].m_cur_cluster_index) return "refine: a block's current cluster is not in its candidate window";
        t.block_cur[b] = (uint32_t)*it;
    }
    t.params.resize(total_clusters);
    for (uint32_t i = 0; i < total_clusters; i++)
        t.params[i] = clusters[i].m_unscaled_color.r | (clusters[i].m_unscaled_color.g << 8) | (clusters[i].m_unscaled_color.b << 16) | ((uint32_t)clusters[i].m_etc_inten << 24);
    out = std::move(t);
    return nullptr;
}

// ---- find_optimal_selector_clusters_for_each_block (fosc_block_struct / fosc_selector_struct, frontend.cpp:2436-2480)

struct fosc_tables {
    std::vector<uint64_t> selector_blocks;   // per POSITION of the flat selector array: an etc_block whose selector bytes hold the entry (memory order)
    std::vector<uint64_t> encoded_blocks;    // per block: the etc_block of its colour5 + inten, selectors zero (memory order)
    windows win;
};

inline const char* translate_fosc(const bu_fosc_block* info, uint32_t n_blocks, uint32_t total_selectors, const bu_fosc_selector* selectors, fosc_tables& out) {
    if ((n_blocks && !info) || (total_selectors && !selectors)) return "fosc: null pointer";
    fosc_tables t;
    if (const char* e = build_windows(n_blocks, total_selectors, [&](uint32_t b, uint32_t& f, uint32_t& c) { f = info[b].m_first_selector; c = info[b].m_num_selectors; }, t.win,
                                      "fosc: candidate window past the end of the selector list", "fosc: empty candidate window",
                                      "fosc: more than 255 distinct candidate windows"))
        return e;
    t.selector_blocks.resize(total_selectors);
    for (uint32_t i = 0; i < total_selectors; i++) t.selector_blocks[i] = selectors_to_etc_block(selectors[i].m_packed_selectors);
    t.encoded_blocks.resize(n_blocks);
    for (uint32_t b = 0; b < n_blocks; b++) {
        const bu_color_rgba c = info[b].m_etc_color5_inten;
        t.encoded_blocks[b] = color5_inten_to_etc_block(c.r, c.g, c.b, c.a);
    }
    out = std::move(t);
    return nullptr;
}

// ---- encode_etc1s_pixel_clusters (cl_pixel_cluster, frontend.cpp:1380-1470): weighted colour lists -> unweighted 8-texel training vectors

// The device layer fits unweighted texel lists made of "training vectors" of 8 texels. A cluster's colours are written out weight_i times each, in list
// order; where the total n is no multiple of 8 the WHOLE list is written reps = 8 / gcd(n, 8) times over, so that reps * n is. Every error is then reps
// times the list's, the (colour5, table) argmin is unchanged, and so are the float mean and the min/max the optimizer starts from while 255 * n * reps
// stays below 2^24 (float sums exact); beyond that the mean is a sum of rounded adds and parity with the unrepeated list is a property of the input.
struct pixel_tables {
    std::vector<uint32_t> texels;      // RGBA words, 8 per training vector, padded with zeros to a multiple of 16
    std::vector<uint32_t> offsets;     // CSR over training vectors: total_clusters + 1
    std::vector<uint32_t> indices;     // training-vector indices of every cluster (consecutive)
    std::vector<uint32_t> reps;        // per cluster: 1, 2, 4 or 8
    std::vector<uint64_t> totals;      // per cluster: n = the sum of its weights
};

inline const char* translate_pixel_clusters(uint32_t total_clusters, const bu_pixel_cluster* clusters, uint64_t total_pixels, const bu_color_rgba* pixels,
                                            const uint32_t* weights, pixel_tables& out) {
    if ((total_clusters && !clusters) || (total_pixels && (!pixels || !weights))) return "pixel clusters: null pointer";
    pixel_tables t;
    t.reps.resize(total_clusters); t.totals.resize(total_clusters);
    uint64_t texels = 0;
    for (uint32_t c = 0; c < total_clusters; c++) {   // everything is checked before anything is expanded
        const uint64_t first = clusters[c].m_first_pixel_index, cnt = clusters[c].m_total_pixels;
        if (first > total_pixels || cnt > total_pixels - first) return "pixel cluster out of range";
        uint64_t n = 0;
        for (uint64_t i = 0; i < cnt; i++) n += weights[first + i];
        if (!n) return "empty pixel cluster";
        uint32_t gcd = 8; while (n % gcd) gcd >>= 1;
        const uint32_t reps = 8 / gcd;
        if (n * reps > 0x7FFFFFFFull) return "pixel cluster too large";
        texels += n * reps;
        if (texels > MAX_EXPANDED_TEXELS) return "pixel clusters: more than 2^31 - 1 texels after expansion";
        t.reps[c] = reps; t.totals[c] = n;
    }
    t.texels.reserve((size_t)((texels + 15) / 16 * 16));
    t.offsets.assign(total_clusters + 1, 0);
    t.indices.reserve((size_t)(texels / 8));
    for (uint32_t c = 0; c < total_clusters; c++) {
        const uint64_t first = clusters[c].m_first_pixel_index, cnt = clusters[c].m_total_pixels;
        const size_t base = t.texels.size();
        for (uint32_t r = 0; r < t.reps[c]; r++)
            for (uint64_t i = 0; i < cnt; i++) {
                uint32_t w; std::memcpy(&w, &pixels[first + i], 4);
                t.texels.insert(t.texels.end(), weights[first + i], w);
            }
        const uint32_t tv_first = (uint32_t)(base / 8), tv_cnt = (uint32_t)((t.texels.size() - base) / 8);
        t.offsets[c + 1] = t.offsets[c] + tv_cnt;
        for (uint32_t v = 0; v < tv_cnt; v++) t.indices.push_back(tv_first + v);
    }
    t.texels.resize((t.texels.size() + 15) / 16 * 16, 0);
    out = std::move(t);
    return nullptr;
}

}  // namespace seam
}  // namespace bu
