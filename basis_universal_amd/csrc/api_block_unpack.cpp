// api_block_unpack.cpp -- the block unpacker behind the C ABI of libbasisu_hip.so: resident BC1 / BC3 / BC4 / BC5 / BC7 blocks -> RGBA8 raster.
#include "api_internal.h"
#include "block_unpack_kernels.h"

static const char* const kUnpackFormats = "BC1_RGB (2), BC3_RGBA (3), BC4_R (4), BC5_RG (5), BC7_RGBA (6)";

extern "C" {

size_t bu_hip_unpack_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t pitch_px, uint32_t rows_px) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_w, orig_h, pitch_px, rows_px }, 4, true);
}

int bu_hip_k_unpack_blocks(bu_hip_context* ctx, const void* d_blocks, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t format, void* d_out,
                           uint32_t pitch_px, uint32_t rows_px, uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    const uint32_t unit = bu::block_unpack_bytes_per_block(format);
    if (!unit) {
        set_error(ctx, "unpack_blocks: format %u (%s) is not supported (supported: %s)", format, transcoder_format_name(format), kUnpackFormats);
        return 0;
    }
    if (!d_blocks || !d_out) { set_error(ctx, "unpack_blocks: null device pointer"); return 0; }
    if (((uintptr_t)d_blocks & (unit - 1)) || ((uintptr_t)d_out & 3u)) {
        set_error(ctx, "unpack_blocks: %s blocks must be %u-byte aligned and the raster 4-byte aligned", transcoder_format_name(format), unit);
        return 0;
    }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry("unpack_blocks", nbx, nby, orig_w, orig_h, pitch_px, rows_px, bu::kEachWay16384, &geo, e); })) return 0;
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    const bu::block_unpack_args a = { d_blocks, static_cast<uint32_t*>(d_out), static_cast<uint32_t*>(counter.p), geo };
    {
        prof_scope ps(ctx, "unpack_blocks");
        BU_TRY(ctx, bu::launch_unpack_blocks(ctx->stream, a, format));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

} // extern "C"
