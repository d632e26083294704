// api_dds_pack.cpp -- the DDS payload packers behind the C ABI of libbasisu_hip.so: resident tiles -> BC1-BC5 blocks, or the tight rows of a raw pixel format.
// Everything is checked before anything is copied or launched: a refused call writes nothing.
#include "api_internal.h"
#include "dds_pack_kernels.h"

static const char* const kFormatNames[] = { "bc1", "bc2", "bc3", "bc4", "bc5", "bc7", "a8r8g8b8", "a8b8g8r8", "r8", "r8g8", "r5g6b5", "a1r5g5b5", "a4r4g4b4" };
static const uint32_t kFormats = sizeof(kFormatNames) / sizeof(kFormatNames[0]);
static const char* const kBlockFormats = "bc1 (0), bc2 (1), bc3 (2), bc4 (3), bc5 (4)";
static const char* const kPixelFormats = "a8r8g8b8 (6), a8b8g8r8 (7), r8 (8), r8g8 (9), r5g6b5 (10), a1r5g5b5 (11), a4r4g4b4 (12)";

// the refusals by format that both entries share; `blocks`: the entry takes block formats
static int check_format(bu_hip_context* ctx, const char* fn, uint32_t format, bool blocks) {
    if (format == BU_HIP_DDS_BC7) {
        set_error(ctx, "%s: format 5 (bc7) is not supported: neither of the reference's two BC7 packers (bc7f, bc7e_scalar) is implemented here", fn);
        return 0;
    }
    if (format >= kFormats) { set_error(ctx, "%s: format %u is unknown (block formats: %s; pixel formats: %s)", fn, format, kBlockFormats, kPixelFormats); return 0; }
    if (bu::dds_pack_is_block_format(format) != blocks) {
        set_error(ctx, "%s: format %u (%s) is a %s format: this entry takes %s", fn, format, kFormatNames[format], blocks ? "pixel" : "block", blocks ? kBlockFormats : kPixelFormats);
        return 0;
    }
    return 1;
}

static int check_buffers(bu_hip_context* ctx, const char* fn, const void* d_tiles, uint64_t n_tiles, const void* d_out) {
    if (!d_tiles || !d_out) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if (((uintptr_t)d_tiles & 15u) || ((uintptr_t)d_out & 15u)) { set_error(ctx, "%s: the tiles and the output must be 16-byte aligned", fn); return 0; }
    if (n_tiles > ((uint64_t)1 << 30)) { set_error(ctx, "%s: %llu tiles: more than 2^30 in one call", fn, (unsigned long long)n_tiles); return 0; }
    return 1;
}

// a record's size with its zeros filled in
static void slice_size(const bu_hip_transcode_slice& s, uint32_t& width, uint32_t& height) {
    width = s.orig_width ? s.orig_width : s.num_blocks_x * 4;
    height = s.orig_height ? s.orig_height : s.num_blocks_y * 4;
}

extern "C" {

size_t bu_hip_dds_payload_bytes(const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t format) {
    const size_t unit = bu::dds_pack_unit_bytes(format);
    if (!slices || !unit) return 0;
    size_t total = 0;
    for (uint32_t i = 0; i < n_slices; i++) {
        uint32_t width, height;
        slice_size(slices[i], width, height);
        total += (bu::dds_pack_is_block_format(format) ? (size_t)slices[i].num_blocks_x * slices[i].num_blocks_y : (size_t)width * height) * unit;
    }
    return total;
}

int bu_hip_k_pack_dds_blocks(bu_hip_context* ctx, const void* d_tiles, uint64_t n_tiles, uint32_t format, void* d_out) {
    if (!ctx) return 0;
    static const char* const fn = "pack_dds_blocks";
    if (!check_format(ctx, fn, format, true) || !check_buffers(ctx, fn, d_tiles, n_tiles, d_out)) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "dds_pack_blocks");
    BU_TRY(ctx, bu::launch_dds_pack_blocks(ctx->stream, d_tiles, (uint32_t)n_tiles, format, d_out));
    return 1;
}

int bu_hip_k_pack_dds_pixels(bu_hip_context* ctx, const void* d_tiles, uint64_t n_tiles, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t format,
                             void* d_out, size_t out_bytes) {
    if (!ctx) return 0;
    static const char* const fn = "pack_dds_pixels";
    if (!check_format(ctx, fn, format, false) || !check_buffers(ctx, fn, d_tiles, n_tiles, d_out)) return 0;
    if (!n_slices) { set_error(ctx, "%s: no slices (n_slices == 0)", fn); return 0; }
    if (!slices) { set_error(ctx, "%s: null pointer", fn); return 0; }
    const uint32_t unit = bu::dds_pack_unit_bytes(format);
    // the table as transcode_slices.h walks it: the records, then the prefix of their tile counts; no counters behind them
    transcode_slice_table table;
    table.n = n_slices;
    table.prefix_at = (size_t)n_slices * sizeof(bu_hip_transcode_slice);
    table.counters_at = table.prefix_at + ((size_t)n_slices + 1) * sizeof(uint32_t);
    table.pack.assign(table.counters_at, 0);
    bu_hip_transcode_slice* rec = reinterpret_cast<bu_hip_transcode_slice*>(table.pack.data());
    uint32_t* prefix = reinterpret_cast<uint32_t*>(table.pack.data() + table.prefix_at);
    uint64_t total = 0, end = 0;
    for (uint32_t i = 0; i < n_slices; i++) {
        bu_hip_transcode_slice s = slices[i];
        if (!s.num_blocks_x || !s.num_blocks_y) { set_error(ctx, "%s: slice %u: zero blocks (%u x %u)", fn, i, s.num_blocks_x, s.num_blocks_y); return 0; }
        if (s.num_blocks_x > 16384u || s.num_blocks_y > 16384u) {
            set_error(ctx, "%s: slice %u: %u x %u blocks is too many (16384 each way at the most)", fn, i, s.num_blocks_x, s.num_blocks_y); return 0;
        }
        slice_size(s, s.orig_width, s.orig_height);
        if (s.orig_width > s.num_blocks_x * 4 || s.orig_height > s.num_blocks_y * 4) {
            set_error(ctx, "%s: slice %u: %u x %u pixels do not fit %u x %u blocks", fn, i, s.orig_width, s.orig_height, s.num_blocks_x, s.num_blocks_y); return 0;
        }
        if (s.out_row_pitch_pixels || s.out_rows_pixels) {
            set_error(ctx, "%s: slice %u: row pitch %u / rows %u given: the rows of a DDS subresource are tight", fn, i, s.out_row_pitch_pixels, s.out_rows_pixels); return 0;
        }
        if (s.alpha_first_block != BU_HIP_NO_ALPHA_SLICE) { set_error(ctx, "%s: slice %u: alpha_first_block is set, and a tile carries its own alpha", fn, i); return 0; }
        const uint64_t tiles = (uint64_t)s.num_blocks_x * s.num_blocks_y, extent = (uint64_t)s.orig_width * s.orig_height * unit;
        if (s.first_block > n_tiles || tiles > n_tiles - s.first_block) {
            set_error(ctx, "%s: slice %u: tiles %llu..%llu are past the %llu given", fn, i, (unsigned long long)s.first_block, (unsigned long long)(s.first_block + tiles),
                      (unsigned long long)n_tiles);
            return 0;
        }
        if (s.out_offset % unit) { set_error(ctx, "%s: slice %u: out_offset %llu is not a multiple of the pixel size %u", fn, i, (unsigned long long)s.out_offset, unit); return 0; }
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
        s.out_row_pitch_pixels = s.orig_width; s.out_rows_pixels = s.orig_height;
        prefix[i] = (uint32_t)total;
        total += tiles;
        if (total > ((uint64_t)1 << 30)) { set_error(ctx, "%s: more than 2^30 tiles in one call (at slice %u)", fn, i); return 0; }
        rec[i] = s;
    }
    prefix[n_slices] = (uint32_t)total;
    table.total_blocks = (uint32_t)total;
    device_guard g(ctx->device);
    if (!table.upload(ctx)) return 0;
    prof_scope ps(ctx, "dds_pack_pixels");
    BU_TRY(ctx, bu::launch_dds_pack_pixels(ctx->stream, d_tiles, table.d_slices, table.d_prefix, n_slices, table.total_blocks, format, d_out));
    return 1;
}

} // extern "C"
