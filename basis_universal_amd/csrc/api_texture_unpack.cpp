// api_texture_unpack.cpp -- the texture unpacker behind the C ABI of libbasisu_hip.so: resident blocks of every format the transcoders write -> RGBA8 raster.
// A family of its own beside api_block_unpack.cpp, whose entry keeps its five formats and its refusals.
#include "api_internal.h"
#include "texture_unpack_kernels.h"

static const char* const kTextureUnpackFormats =
    "ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC3_RGBA (3), BC4_R (4), BC5_RG (5), BC7_RGBA (6), PVRTC1_4_RGB (8), PVRTC1_4_RGBA (9), ASTC_4x4_RGBA (10), "
    "ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21)";

static bool is_pow2(uint32_t v) { return v && !(v & (v - 1u)); }

extern "C" {

uint32_t bu_hip_unpack_texture_bytes_per_block(uint32_t format) { return bu::texture_unpack_bytes_per_block(format); }

int bu_hip_k_unpack_texture(bu_hip_context* ctx, const void* d_blocks, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t format, void* d_out,
                            uint32_t pitch_px, uint32_t rows_px, uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    const uint32_t unit = bu::texture_unpack_bytes_per_block(format);
    if (!unit) {
        set_error(ctx, "unpack_texture: format %u (%s) is not supported (supported: %s)", format, transcoder_format_name(format), kTextureUnpackFormats);
        return 0;
    }
    if (!d_blocks || !d_out) { set_error(ctx, "unpack_texture: null device pointer"); return 0; }
    if (((uintptr_t)d_blocks & (unit - 1)) || ((uintptr_t)d_out & 3u)) {
        set_error(ctx, "unpack_texture: %s blocks must be %u-byte aligned and the raster 4-byte aligned", transcoder_format_name(format), unit);
        return 0;
    }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry("unpack_texture", nbx, nby, orig_w, orig_h, pitch_px, rows_px, bu::kEachWay16384, &geo, e); })) return 0;
    if ((format == 8u || format == 9u) && nbx && nby && (!is_pow2(geo.width) || !is_pow2(geo.height) || !is_pow2(nbx) || !is_pow2(nby))) {
        set_error(ctx, "unpack_texture: %u x %u pixels in %u x %u blocks: PVRTC1 only supports power of 2 dimensions", geo.width, geo.height, nbx, nby);
        return 0;
    }
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    const bu::texture_unpack_args a = { d_blocks, static_cast<uint32_t*>(d_out), static_cast<uint32_t*>(counter.p), geo };
    {
        prof_scope ps(ctx, "unpack_texture");
        BU_TRY(ctx, bu::launch_unpack_texture(ctx->stream, a, format));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

} // extern "C"
