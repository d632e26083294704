// api_transcode_slices.cpp -- the slice table of the two whole-file transcoders (bu_hip_k_transcode_uastc_slices in api_uastc.cpp, bu_hip_k_transcode_etc1s_slices in
// api_etc1s_transcode.cpp): the refusals they share, the one upload, the one read-back.
#include "api_internal.h"
#include "etc1s_transcode_kernels.h"
#include "uastc_transcode_kernels.h"

static const uint32_t kUastcRGBA32 = 13;   // cTFRGBA32: UASTC's one pixel target

// bytes per pixel of a pixel target, else 0
static uint32_t pixel_unit(uint32_t target, bool etc1s) {
    if (etc1s) return bu::etc1s_transcode_is_pixel_target(target) ? bu::etc1s_transcode_unit_bytes(target) : 0u;
    return target == kUastcRGBA32 ? 4u : 0u;
}
static uint32_t block_unit(uint32_t target, bool etc1s) {
    if (etc1s) return bu::etc1s_transcode_is_pixel_target(target) ? 0u : bu::etc1s_transcode_unit_bytes(target);
    return target == kUastcRGBA32 ? 0u : (uint32_t)bu::transcode_output_bytes(1, 1, 0, 0, target);
}

extern "C" size_t bu_hip_transcode_slice_extent(const bu_hip_transcode_slice* s, uint32_t target, int etc1s) {
    if (!s) return 0;
    if (const size_t unit = block_unit(target, etc1s != 0)) return (size_t)s->num_blocks_x * s->num_blocks_y * unit;
    const size_t unit = pixel_unit(target, etc1s != 0);
    const size_t width = s->orig_width ? s->orig_width : (size_t)s->num_blocks_x * 4, height = s->orig_height ? s->orig_height : (size_t)s->num_blocks_y * 4;
    return (s->out_row_pitch_pixels ? s->out_row_pitch_pixels : width) * (s->out_rows_pixels ? s->out_rows_pixels : height) * unit;
}

int transcode_slice_table::check(bu_hip_context* ctx, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target, bool etc1s,
                                 const void* d_out, size_t out_bytes) {
    static_assert(sizeof(bu_hip_transcode_slice) == 48, "the kernels read a record as three 16-byte words");
    if (!n_slices) { set_error(ctx, "%s: no slices (n_slices == 0)", fn); return 0; }
    if (!slices || !d_out) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if ((uintptr_t)d_out & 15u) { set_error(ctx, "%s: the output is not 16-byte aligned", fn); return 0; }
    const bool pixels = pixel_unit(target, etc1s) != 0;
    const char* const inputs = etc1s ? "indices" : "blocks";
    n = n_slices;
    prefix_at = (size_t)n * sizeof(bu_hip_transcode_slice);
    counters_at = prefix_at + ((size_t)n + 1) * sizeof(uint32_t);
    pack.assign(counters_at + (size_t)n * sizeof(uint32_t), 0);
    bu_hip_transcode_slice* rec = reinterpret_cast<bu_hip_transcode_slice*>(pack.data());
    uint32_t* prefix = reinterpret_cast<uint32_t*>(pack.data() + prefix_at);
    uint64_t total = 0, end = 0;
    for (uint32_t i = 0; i < n; i++) {
        bu_hip_transcode_slice s = slices[i];
        if (!s.num_blocks_x || !s.num_blocks_y) { set_error(ctx, "%s: slice %u: zero blocks (%u x %u)", fn, i, s.num_blocks_x, s.num_blocks_y); return 0; }
        if (s.num_blocks_x > 16384u || s.num_blocks_y > 16384u) {
            set_error(ctx, "%s: slice %u: %u x %u blocks is too many (16384 each way at the most)", fn, i, s.num_blocks_x, s.num_blocks_y); return 0;
        }
        if (!s.orig_width) s.orig_width = s.num_blocks_x * 4;
        if (!s.orig_height) s.orig_height = s.num_blocks_y * 4;
        if (s.orig_width > s.num_blocks_x * 4 || s.orig_height > s.num_blocks_y * 4) {
            set_error(ctx, "%s: slice %u: %u x %u pixels do not fit %u x %u blocks", fn, i, s.orig_width, s.orig_height, s.num_blocks_x, s.num_blocks_y); return 0;
        }
        if (!pixels && (s.out_row_pitch_pixels || s.out_rows_pixels)) {
            set_error(ctx, "%s: slice %u: row pitch %u / rows %u given for a block target (%s): they describe a pixel raster", fn, i, s.out_row_pitch_pixels, s.out_rows_pixels,
                      transcoder_format_name(target));
            return 0;
        }
        const size_t extent = bu_hip_transcode_slice_extent(&s, target, etc1s);   // before the zeros of pitch / rows are filled in: a block target's stay 0
        if (!s.out_row_pitch_pixels) s.out_row_pitch_pixels = s.orig_width;
        if (!s.out_rows_pixels) s.out_rows_pixels = s.orig_height;
        if (s.out_row_pitch_pixels < s.orig_width) { set_error(ctx, "%s: slice %u: row pitch %u is less than the width %u", fn, i, s.out_row_pitch_pixels, s.orig_width); return 0; }
        const uint64_t blocks = (uint64_t)s.num_blocks_x * s.num_blocks_y;
        if (!etc1s && s.alpha_first_block != BU_HIP_NO_ALPHA_SLICE) { set_error(ctx, "%s: slice %u: alpha_first_block is set, and a UASTC image has no alpha slice", fn, i); return 0; }
        if (s.first_block > n_inputs || blocks > n_inputs - s.first_block) {
            set_error(ctx, "%s: slice %u: %s %llu..%llu are past the %llu given", fn, i, inputs, (unsigned long long)s.first_block, (unsigned long long)(s.first_block + blocks),
                      (unsigned long long)n_inputs);
            return 0;
        }
        if (s.alpha_first_block != BU_HIP_NO_ALPHA_SLICE && (s.alpha_first_block > n_inputs || blocks > n_inputs - s.alpha_first_block)) {
            set_error(ctx, "%s: slice %u: alpha %s %llu..%llu are past the %llu given", fn, i, inputs, (unsigned long long)s.alpha_first_block,
                      (unsigned long long)(s.alpha_first_block + blocks), (unsigned long long)n_inputs);
            return 0;
        }
        if (s.out_offset & 15u) { set_error(ctx, "%s: slice %u: out_offset %llu is not 16-byte aligned", fn, i, (unsigned long long)s.out_offset); return 0; }
        if (s.out_offset < end) {
            set_error(ctx, "%s: slice %u: out_offset %llu lies before the end of slice %u's output (%llu): outputs must ascend without overlap", fn, i,
                      (unsigned long long)s.out_offset, i ? i - 1 : 0, (unsigned long long)end);
            return 0;
        }
        if (s.out_offset > out_bytes || extent > out_bytes - s.out_offset) {
            set_error(ctx, "%s: slice %u: its output, bytes %llu..%llu, ends past out_bytes = %llu", fn, i, (unsigned long long)s.out_offset,
                      (unsigned long long)(s.out_offset + extent), (unsigned long long)out_bytes);
            return 0;
        }
        end = s.out_offset + extent;
        prefix[i] = (uint32_t)total;
        total += blocks;
        if (total > ((uint64_t)1 << 30)) { set_error(ctx, "%s: more than 2^30 blocks in one call (at slice %u)", fn, i); return 0; }
        rec[i] = s;
    }
    prefix[n] = (uint32_t)total;
    total_blocks = (uint32_t)total;
    return 1;
}

int transcode_slice_table::upload(bu_hip_context* ctx) {
    arena& table = ctx->scratch[4];
    BU_TRY(ctx, table.reserve(pack.size()));
    BU_TRY(ctx, h2d(ctx, table.p, pack.data(), counters_at));   // the counters are cleared on the device
    const uint8_t* base = static_cast<const uint8_t*>(table.p);
    d_slices = reinterpret_cast<const bu_hip_transcode_slice*>(base);
    d_prefix = reinterpret_cast<const uint32_t*>(base + prefix_at);
    d_counters = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(table.p) + counters_at);
    return 1;
}

int transcode_slice_table::read_counters(bu_hip_context* ctx, uint32_t* out_per_slice) {
    BU_TRY(ctx, d2h_pageable(ctx, out_per_slice, d_counters, (size_t)n * sizeof(uint32_t)));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}
