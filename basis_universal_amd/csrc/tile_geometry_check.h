// tile_geometry_check.h -- the host half of tile_raster.h: what the entries of the C ABI that move tiles into or out of a raster check before anything is copied or
// launched, written once. Plain C++: no HIP header, no context. A refusal is a sentence in the caller's buffer and a return of 0 (api_internal.h forwards it to
// set_error), so the same code runs in the CPU suite (tests/native/tile_geometry_host.cpp).
//   resolve_geometry   : one image -- the zeros of width / height / pitch / rows, too many blocks, pixels that do not fit the blocks, a pitch below the width
//   raster_output_bytes: the bytes such an image's output takes
//   slice_table        : the pack one launch over many slices reads (records, prefix of their item counts, optional counters), its 2^30 limit and the "ranges ascend
//                        without overlap" rule; build_transcode_slices (the whole-file transcoders, the DDS pixel packer) and build_source_slices (extract_slices)
//                        are the per-record checks in front of it
//   raster_pair_region : the two rasters of a quality metric
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "tile_raster.h"

namespace bu {

struct err_text { char* text; size_t size; };   // where a refusal is written
typedef unsigned long long ull;

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline int refuse(err_text err, const char* fmt, ...) {   // always 0
    va_list ap;
    va_start(ap, fmt);
    if (err.text && err.size) vsnprintf(err.text, err.size, fmt, ap);
    va_end(ap);
    return 0;
}

// What differs between callers in "too many blocks": transcode_uastc takes any grid of up to 2^31 - 1 blocks, everyone else 16384 blocks each way.
struct geometry_limits { uint32_t each_way; uint64_t in_all; };
inline constexpr geometry_limits kEachWay16384 = { 16384u, 0 }, kUastcOneImage = { 0, 0x7FFFFFFFull };

// `who` begins every sentence ("unpack_blocks", "transcode_etc1s_slices: slice 3"). orig_w / orig_h 0 = 4 * blocks; pitch / rows 0 = width / height.
inline int resolve_geometry(const char* who, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t pitch, uint32_t rows, const geometry_limits& limits,
                            tile_geometry* g, err_text err) {
    if (limits.in_all && (uint64_t)nbx * nby > limits.in_all) return refuse(err, "%s: %u x %u blocks is too many", who, nbx, nby);
    if (limits.each_way && (nbx > limits.each_way || nby > limits.each_way))
        return refuse(err, "%s: %u x %u blocks is too many (%u each way at the most)", who, nbx, nby, limits.each_way);
    const uint32_t width = orig_w ? orig_w : nbx * 4, height = orig_h ? orig_h : nby * 4;
    if (width > nbx * 4 || height > nby * 4) return refuse(err, "%s: %u x %u pixels do not fit %u x %u blocks", who, width, height, nbx, nby);
    *g = tile_geometry{ nbx, nby, width, height, pitch ? pitch : width, rows ? rows : height };
    if (g->pitch < width) return refuse(err, "%s: row pitch %u is less than the width %u", who, g->pitch, width);
    return 1;
}

// Bytes the output of one image takes; g may still hold the caller's zeros. Block targets: `unit` bytes per block; pixel targets: pitch x rows pixels of `unit` bytes.
// two_wide: a block target whose blocks cover two tiles side by side (FXT1): rows of (nbx + 1) / 2 blocks.
inline size_t raster_output_bytes(const tile_geometry& g, size_t unit, bool is_pixel_target, bool two_wide = false) {
    if (!is_pixel_target) return (two_wide ? ((size_t)g.nbx + 1) / 2 : (size_t)g.nbx) * g.nby * unit;
    const size_t width = g.width ? g.width : (size_t)g.nbx * 4, height = g.height ? g.height : (size_t)g.nby * 4;
    return (g.pitch ? g.pitch : width) * (g.rows ? g.rows : height) * unit;
}

// The pack of a launch over many slices, as it goes up in one copy: n records, prefix[n + 1] (where each slice's items -- blocks, tiles -- begin among all items of
// the call; prefix[n] = total), and behind them room for n counters the launcher clears on the device (upload_bytes() stops before them).
struct slice_table {
    std::vector<uint8_t> pack;
    size_t record_bytes = 0, prefix_at = 0, counters_at = 0;
    uint32_t n = 0, total = 0;

    void begin(uint32_t n_slices, size_t bytes_per_record, bool counters) {
        n = n_slices; record_bytes = bytes_per_record; total = 0; sum = end = 0;
        prefix_at = (size_t)n * record_bytes;
        counters_at = prefix_at + ((size_t)n + 1) * sizeof(uint32_t);
        pack.assign(counters_at + (counters ? (size_t)n * sizeof(uint32_t) : 0), 0);
    }
    size_t upload_bytes() const { return counters_at; }
    const uint32_t* prefix() const { return reinterpret_cast<const uint32_t*>(pack.data() + prefix_at); }
    // slice i takes [first, first + extent) of something (`field` names the record's member, `whose` / `plural` what it holds): refused where it begins before slice i - 1 ended
    int ascends(const char* fn, uint32_t i, const char* field, const char* whose, const char* plural, uint64_t first, uint64_t extent, err_text err) {
        if (first < end)
            return refuse(err, "%s: slice %u: %s %llu lies before the end of slice %u's %s (%llu): %s must ascend without overlap", fn, i, field, (ull)first, i ? i - 1 : 0, whose,
                          (ull)end, plural);
        end = first + extent;
        return 1;
    }
    // record i as it is uploaded, and its `items` items (>= 1) of the call's 2^30
    int add(const char* fn, uint32_t i, const void* record, uint64_t items, const char* item_name, err_text err) {
        uint32_t* p = reinterpret_cast<uint32_t*>(pack.data() + prefix_at);
        p[i] = (uint32_t)sum;
        sum += items;
        if (sum > ((uint64_t)1 << 30)) return refuse(err, "%s: more than 2^30 %s in one call (at slice %u)", fn, item_name, i);
        memcpy(pack.data() + (size_t)i * record_bytes, record, record_bytes);
        p[i + 1] = total = (uint32_t)sum;
        return 1;
    }
private:
    uint64_t sum = 0, end = 0;
};

// What differs between the callers of build_transcode_slices.
struct slice_policy {
    const char *inputs, *items;   // what first_block counts ("blocks", "indices", "tiles"), and what the 2^30 of one call are ("blocks", "tiles")
    uint32_t unit;                // bytes per block of a block target, per pixel of a pixel target
    bool pixels;
    bool offsets_in_pixels;       // out_offset: a multiple of the pixel size (tight subresources of odd sizes) instead of 16
    char pitch_refusal[96];       // "" = a pitch / rows may be given; else how the sentence "row pitch %u / rows %u given" goes on
    const char* alpha_refusal;    // nullptr = an alpha slice may be given; else how "alpha_first_block is set, and " goes on
    bool counters;
    bool two_wide;                // a block target whose blocks cover two tiles side by side (FXT1)
};

// the whole-file transcoders: pitch / rows for pixel targets only, an alpha slice for ETC1S only, a counter per slice
inline slice_policy transcoder_slice_policy(bool etc1s, uint32_t unit, bool pixels, const char* target_name) {
    slice_policy p = { etc1s ? "indices" : "blocks", "blocks", unit, pixels, false, "", etc1s ? nullptr : "a UASTC image has no alpha slice", true, false };
    if (!pixels) snprintf(p.pitch_refusal, sizeof(p.pitch_refusal), " for a block target (%s): they describe a pixel raster", target_name);
    return p;
}
// the DDS pixel packer: tight rows, tiles that carry their own alpha, nothing counted
inline slice_policy dds_pixels_slice_policy(uint32_t unit) {
    return slice_policy{ "tiles", "tiles", unit, true, true, ": the rows of a DDS subresource are tight", "a tile carries its own alpha", false, false };
}

// Every refusal of a table of bu_hip_transcode_slice records, and the pack: the records with their zero sizes filled in. Nothing else is touched.
inline int build_transcode_slices(slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, const slice_policy& p,
                                  const void* d_out, size_t out_bytes, err_text err) {
    static_assert(sizeof(bu_hip_transcode_slice) == 48, "the kernels read a record as three 16-byte words");
    if (!n_slices) return refuse(err, "%s: no slices (n_slices == 0)", fn);
    if (!slices || !d_out) return refuse(err, "%s: null pointer", fn);
    if ((uintptr_t)d_out & 15u) return refuse(err, "%s: the output is not 16-byte aligned", fn);
    t.begin(n_slices, sizeof(bu_hip_transcode_slice), p.counters);
    for (uint32_t i = 0; i < n_slices; i++) {
        bu_hip_transcode_slice s = slices[i];
        char who[96];
        snprintf(who, sizeof(who), "%s: slice %u", fn, i);
        if (!s.num_blocks_x || !s.num_blocks_y) return refuse(err, "%s: zero blocks (%u x %u)", who, s.num_blocks_x, s.num_blocks_y);
        // a pitch / rows that the policy refuses is refused by its own sentence, after the sizes': resolve_geometry sees none
        const bool no_pitch = p.pitch_refusal[0] != 0;
        tile_geometry g;
        if (!resolve_geometry(who, s.num_blocks_x, s.num_blocks_y, s.orig_width, s.orig_height, no_pitch ? 0 : s.out_row_pitch_pixels, no_pitch ? 0 : s.out_rows_pixels,
                              kEachWay16384, &g, err)) return 0;
        if (no_pitch && (s.out_row_pitch_pixels || s.out_rows_pixels))
            return refuse(err, "%s: row pitch %u / rows %u given%s", who, s.out_row_pitch_pixels, s.out_rows_pixels, p.pitch_refusal);
        const bool alpha = s.alpha_first_block != BU_HIP_NO_ALPHA_SLICE;
        if (alpha && p.alpha_refusal) return refuse(err, "%s: alpha_first_block is set, and %s", who, p.alpha_refusal);
        const uint64_t blocks = (uint64_t)g.nbx * g.nby, extent = raster_output_bytes(g, p.unit, p.pixels, p.two_wide);
        if (s.first_block > n_inputs || blocks > n_inputs - s.first_block)
            return refuse(err, "%s: %s %llu..%llu are past the %llu given", who, p.inputs, (ull)s.first_block, (ull)(s.first_block + blocks), (ull)n_inputs);
        if (alpha && (s.alpha_first_block > n_inputs || blocks > n_inputs - s.alpha_first_block))
            return refuse(err, "%s: alpha %s %llu..%llu are past the %llu given", who, p.inputs, (ull)s.alpha_first_block, (ull)(s.alpha_first_block + blocks), (ull)n_inputs);
        if (p.offsets_in_pixels) {
            if (s.out_offset % p.unit) return refuse(err, "%s: out_offset %llu is not a multiple of the pixel size %u", who, (ull)s.out_offset, p.unit);
        } else if (s.out_offset & 15u) return refuse(err, "%s: out_offset %llu is not 16-byte aligned", who, (ull)s.out_offset);
        if (!t.ascends(fn, i, "out_offset", "output", "outputs", s.out_offset, extent, err)) return 0;
        if (s.out_offset > out_bytes || extent > out_bytes - s.out_offset)
            return refuse(err, "%s: its output, bytes %llu..%llu, ends past out_bytes = %llu", who, (ull)s.out_offset, (ull)(s.out_offset + extent), (ull)out_bytes);
        s.orig_width = g.width; s.orig_height = g.height; s.out_row_pitch_pixels = g.pitch; s.out_rows_pixels = g.rows;
        if (!t.add(fn, i, &s, blocks, p.items, err)) return 0;
    }
    return 1;
}

// The same for extract_slices' records, which go up as they are: a slice's items are the tiles of its raster, and the ranges that ascend are those of first_block.
inline int build_source_slices(slice_table& t, const char* fn, const bu_hip_slice_source* slices, uint32_t n, const void* d_out, err_text err) {
    static_assert(sizeof(bu_hip_slice_source) == 32, "the kernel reads a record as two 16-byte words");
    if (!n) return refuse(err, "%s: no slices (n == 0)", fn);
    if (!slices || !d_out) return refuse(err, "%s: null pointer", fn);
    if ((uintptr_t)d_out & 15u) return refuse(err, "%s: the output is not 16-byte aligned", fn);
    t.begin(n, sizeof(bu_hip_slice_source), false);
    for (uint32_t i = 0; i < n; i++) {
        const bu_hip_slice_source& s = slices[i];
        if (!s.d_raster) return refuse(err, "%s: slice %u: null raster", fn, i);
        if (!s.width || !s.height) return refuse(err, "%s: slice %u: zero size (%u x %u)", fn, i, s.width, s.height);
        if (s.width > 0x7fffffffu || s.height > 0x7fffffffu) return refuse(err, "%s: slice %u: %u x %u pixels is too large", fn, i, s.width, s.height);
        if ((uint64_t)s.pitch_bytes < (uint64_t)s.width * 4u)
            return refuse(err, "%s: slice %u: row pitch %u bytes is less than 4 * width = %llu", fn, i, s.pitch_bytes, (ull)s.width * 4u);
        if (s.mode > BU_HIP_SLICE_ALPHA) return refuse(err, "%s: slice %u: unknown mode %u", fn, i, s.mode);
        const uint64_t tiles = (((uint64_t)s.width + 3u) / 4u) * (((uint64_t)s.height + 3u) / 4u);
        if (!t.ascends(fn, i, "first_block", "blocks", "ranges", s.first_block, tiles, err) || !t.add(fn, i, &s, tiles, "tiles", err)) return 0;
    }
    return 1;
}

// The two rasters of a quality metric (RGBA8, pitches in pixels, 0 = the width): both 4-byte aligned, each pitch at least its width; the region is what they have in
// common, at most max_dim each way.
inline int raster_pair_region(const char* fn, const void* d_a, uint32_t wa, uint32_t ha, uint32_t* pa, const void* d_b, uint32_t wb, uint32_t hb, uint32_t* pb, uint32_t* w,
                              uint32_t* h, uint32_t max_dim, err_text err) {
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 3u) return refuse(err, "%s: a raster is not 4-byte aligned", fn);
    *pa = *pa ? *pa : wa; *pb = *pb ? *pb : wb;
    if (*pa < wa) return refuse(err, "%s: row pitch %u of the first raster is less than its width %u", fn, *pa, wa);
    if (*pb < wb) return refuse(err, "%s: row pitch %u of the second raster is less than its width %u", fn, *pb, wb);
    *w = std::min(wa, wb); *h = std::min(ha, hb);
    if (*w > max_dim || *h > max_dim) return refuse(err, "%s: a region of %u x %u pixels is too large (%u each way at the most)", fn, *w, *h, max_dim);
    return 1;
}

}  // namespace bu
