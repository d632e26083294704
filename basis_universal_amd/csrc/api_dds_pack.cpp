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

extern "C" {

size_t bu_hip_dds_payload_bytes(const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t format) {
    const size_t unit = bu::dds_pack_unit_bytes(format);
    if (!slices || !unit) return 0;
    size_t total = 0;
    for (uint32_t i = 0; i < n_slices; i++) {
        const bu_hip_transcode_slice& s = slices[i];   // tight rows whatever the record says of pitch / rows
        total += bu::raster_output_bytes(bu::tile_geometry{ s.num_blocks_x, s.num_blocks_y, s.orig_width, s.orig_height, 0, 0 }, unit, !bu::dds_pack_is_block_format(format));
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
    // the table as find_transcode_slice walks it (tile_raster.h): the records, then the prefix of their tile counts; no counters behind them
    bu::slice_table table;
    const bu::slice_policy policy = bu::dds_pixels_slice_policy(bu::dds_pack_unit_bytes(format));
    if (!checked(ctx, [&](bu::err_text e) { return bu::build_transcode_slices(table, fn, slices, n_slices, n_tiles, policy, d_out, out_bytes, e); })) return 0;
    device_guard g(ctx->device);
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    prof_scope ps(ctx, "dds_pack_pixels");
    BU_TRY(ctx, bu::launch_dds_pack_pixels(ctx->stream, d_tiles, static_cast<const bu_hip_transcode_slice*>(d.records), d.prefix, n_slices, table.total, format, d_out));
    return 1;
}

} // extern "C"
