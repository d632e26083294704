// api_source_prep.cpp -- the source-image options of the compressor behind the C ABI of libbasisu_hip.so: prepare (renormalise / swizzle / alpha policy / flip),
// renormalise in place, and the ETC1S alpha split, each one launch over resident RGBA8 rasters.
#include "api_internal.h"
#include "source_prep_kernels.h"

// what every raster argument of this file must satisfy; names the first thing wrong
static bool raster_ok(bu_hip_context* ctx, const char* fn, const char* what, const void* p, uint32_t width, uint32_t pitch_bytes) {
    if (!p) { set_error(ctx, "%s: null device pointer (%s)", fn, what); return false; }
    if (pitch_bytes < width * 4u) { set_error(ctx, "%s: %s row pitch %u bytes is less than 4 * width = %u", fn, what, pitch_bytes, width * 4u); return false; }
    if (((uintptr_t)p & 3u) || (pitch_bytes & 3u)) { set_error(ctx, "%s: the %s raster and its row pitch must be 4-byte aligned", fn, what); return false; }
    return true;
}

static bool size_ok(bu_hip_context* ctx, const char* fn, uint32_t width, uint32_t height) {
    if (!width || !height) { set_error(ctx, "%s: zero dimension (%u x %u)", fn, width, height); return false; }
    if (width > 16384u || height > 16384u) { set_error(ctx, "%s: %u x %u pixels is too large (16384 each way at the most)", fn, width, height); return false; }
    return true;
}

static int prepare(bu_hip_context* ctx, const char* fn, const bu::source_prep_args& args, uint32_t* out_any_below_255) {
    device_guard g(ctx->device);
    arena& word = ctx->scratch[4];
    BU_TRY(ctx, word.reserve(sizeof(uint32_t)));
    bu::source_prep_args a = args;
    a.any_alpha = static_cast<uint32_t*>(word.p);
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_prepare_source(ctx->stream, a));
    }
    if (out_any_below_255) {
        uint32_t any = 0;
        if (!read_back(ctx, &any, word.p, sizeof(any))) return 0;
        *out_any_below_255 = any & 1u;
    }
    return 1;
}

extern "C" {

int bu_hip_k_prepare_source(bu_hip_context* ctx, const void* d_src, uint32_t width, uint32_t height, uint32_t src_pitch_bytes, void* d_dst, uint32_t dst_pitch_bytes,
                            int renormalize, uint32_t swizzle, int check_for_alpha, int force_alpha, int y_flip, uint32_t* out_has_alpha, uint32_t* out_alpha_below_255) {
    if (!ctx) return 0;
    static const char* const fn = "prepare_source";
    if (!d_src || !d_dst) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if (!size_ok(ctx, fn, width, height) || !raster_ok(ctx, fn, "source", d_src, width, src_pitch_bytes) || !raster_ok(ctx, fn, "destination", d_dst, width, dst_pitch_bytes)) return 0;
    if (!bu::source_prep_swizzle_valid(swizzle)) { set_error(ctx, "%s: swizzle entry above 3 (0x%08x; one byte per channel, each 0..3)", fn, swizzle); return 0; }
    if (y_flip && d_src == d_dst) { set_error(ctx, "%s: source equals destination with y_flip set (the flip cannot run in place)", fn); return 0; }
    bu::source_prep_args a = { static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), nullptr, width, height, src_pitch_bytes, dst_pitch_bytes,
                               { renormalize ? 1u : 0u, swizzle, check_for_alpha ? 1u : 0u, force_alpha ? 1u : 0u, y_flip ? 1u : 0u } };
    uint32_t below = 0;
    if (!prepare(ctx, fn, a, &below)) return 0;   // synchronises once, for the flag
    if (out_has_alpha) *out_has_alpha = bu::source_prep_has_alpha(a.o, below != 0u) ? 1u : 0u;
    if (out_alpha_below_255) *out_alpha_below_255 = below;
    return 1;
}

int bu_hip_k_renormalize_normal_map(bu_hip_context* ctx, void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes) {
    if (!ctx) return 0;
    static const char* const fn = "renormalize_normal_map";
    if (!d_rgba) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if (!size_ok(ctx, fn, width, height) || !raster_ok(ctx, fn, "image", d_rgba, width, pitch_bytes)) return 0;
    // alpha is kept whatever it is: the policy's "forced" branch
    bu::source_prep_args a = { static_cast<const uint8_t*>(d_rgba), static_cast<uint8_t*>(d_rgba), nullptr, width, height, pitch_bytes, pitch_bytes,
                               { 1u, bu::SOURCE_PREP_IDENTITY_SWIZZLE, 1u, 1u, 0u } };
    return prepare(ctx, fn, a, nullptr);
}

int bu_hip_k_split_alpha(bu_hip_context* ctx, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out_rgb, uint32_t rgb_pitch_bytes,
                         void* d_out_alpha, uint32_t alpha_pitch_bytes) {
    if (!ctx) return 0;
    static const char* const fn = "split_alpha";
    if (!d_rgba || !d_out_rgb || !d_out_alpha) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if (!size_ok(ctx, fn, width, height) || !raster_ok(ctx, fn, "source", d_rgba, width, pitch_bytes) || !raster_ok(ctx, fn, "colour", d_out_rgb, width, rgb_pitch_bytes) ||
        !raster_ok(ctx, fn, "alpha", d_out_alpha, width, alpha_pitch_bytes)) return 0;
    if (d_out_rgb == d_out_alpha || d_out_alpha == d_rgba) { set_error(ctx, "%s: the alpha plane needs a buffer of its own", fn); return 0; }
    device_guard g(ctx->device);
    const bu::split_alpha_args a = { static_cast<const uint8_t*>(d_rgba), static_cast<uint8_t*>(d_out_rgb), static_cast<uint8_t*>(d_out_alpha), width, height,
                                     pitch_bytes, rgb_pitch_bytes, alpha_pitch_bytes };
    prof_scope ps(ctx, fn);
    BU_TRY(ctx, bu::launch_split_alpha(ctx->stream, a));
    return 1;
}

} // extern "C"
