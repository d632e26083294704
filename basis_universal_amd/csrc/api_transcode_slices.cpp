// api_transcode_slices.cpp -- the slice table of the two whole-file transcoders (bu_hip_k_transcode_uastc_slices in api_uastc.cpp, bu_hip_k_transcode_etc1s_slices in
// api_etc1s_transcode.cpp): which target writes pixels and how large its unit is. The refusals, the pack and the upload are tile_geometry_check.h's and api_internal.h's.
#include "api_internal.h"
#include "etc1s_transcode_kernels.h"
#include "uastc_transcode_kernels.h"

static const uint32_t kUastcRGBA32 = 13;   // cTFRGBA32: UASTC's one pixel target

static bool is_pixel_target(uint32_t target, bool etc1s) { return etc1s ? bu::etc1s_transcode_is_pixel_target(target) : target == kUastcRGBA32; }
// bytes per pixel of a pixel target, per block of a block target; 0 = the codec does not have the target
static uint32_t target_unit(uint32_t target, bool etc1s) {
    if (etc1s) return bu::etc1s_transcode_unit_bytes(target);
    return target == kUastcRGBA32 ? 4u : (uint32_t)bu::transcode_output_bytes(1, 1, 0, 0, target);
}

extern "C" size_t bu_hip_transcode_slice_extent(const bu_hip_transcode_slice* s, uint32_t target, int etc1s) {
    if (!s) return 0;
    const bu::tile_geometry g = { s->num_blocks_x, s->num_blocks_y, s->orig_width, s->orig_height, s->out_row_pitch_pixels, s->out_rows_pixels };
    return bu::raster_output_bytes(g, target_unit(target, etc1s != 0), is_pixel_target(target, etc1s != 0));
}

extern "C" size_t bu_hip_etc1s_image_slice_extent(const bu_hip_transcode_slice* s, uint32_t target) {
    if (!s) return 0;
    const bu::tile_geometry g = { s->num_blocks_x, s->num_blocks_y, s->orig_width, s->orig_height, s->out_row_pitch_pixels, s->out_rows_pixels };
    return bu::raster_output_bytes(g, bu::etc1s_texture_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target));
}

extern "C" size_t bu_hip_etc1s_block_format_slice_extent(const bu_hip_transcode_slice* s, uint32_t target) {
    if (!s) return 0;
    const bu::tile_geometry g = { s->num_blocks_x, s->num_blocks_y, s->orig_width, s->orig_height, s->out_row_pitch_pixels, s->out_rows_pixels };
    return bu::raster_output_bytes(g, bu::etc1s_block_format_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target));
}

extern "C" size_t bu_hip_etc1s_vendor_format_slice_extent(const bu_hip_transcode_slice* s, uint32_t target) {
    if (!s) return 0;
    const bu::tile_geometry g = { s->num_blocks_x, s->num_blocks_y, s->orig_width, s->orig_height, s->out_row_pitch_pixels, s->out_rows_pixels };
    return bu::raster_output_bytes(g, bu::etc1s_vendor_format_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target), target == bu::ETF_FXT1_RGB);
}

extern "C" size_t bu_hip_uastc_texture_slice_extent(const bu_hip_transcode_slice* s, uint32_t target) {
    if (!s) return 0;
    const bu::tile_geometry g = { s->num_blocks_x, s->num_blocks_y, s->orig_width, s->orig_height, s->out_row_pitch_pixels, s->out_rows_pixels };
    return bu::raster_output_bytes(g, bu::uastc_texture_unit_bytes(target), bu::uastc_texture_is_pixel_target(target));
}

// the UASTC table under the texture family's target list (bu_hip_k_transcode_uastc_textures): four pixel targets, units of 2 to 16 bytes
int uastc_texture_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs,
                               uint32_t target, const void* d_out, size_t out_bytes) {
    const bu::slice_policy p = bu::transcoder_slice_policy(false, bu::uastc_texture_unit_bytes(target), bu::uastc_texture_is_pixel_target(target), transcoder_format_name(target));
    return checked(ctx, [&](bu::err_text e) { return bu::build_transcode_slices(t, fn, slices, n_slices, n_inputs, p, d_out, out_bytes, e); });
}

// the ETC1S table under any of the families' target lists: `unit` is the family's unit for the target (0 = it does not have it)
int etc1s_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target,
                       uint32_t unit, const void* d_out, size_t out_bytes, bool two_wide) {
    bu::slice_policy p = bu::transcoder_slice_policy(true, unit, bu::etc1s_transcode_is_pixel_target(target), transcoder_format_name(target));
    p.two_wide = two_wide;
    return checked(ctx, [&](bu::err_text e) { return bu::build_transcode_slices(t, fn, slices, n_slices, n_inputs, p, d_out, out_bytes, e); });
}

int transcode_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target,
                           bool etc1s, const void* d_out, size_t out_bytes) {
    const bu::slice_policy p = bu::transcoder_slice_policy(etc1s, target_unit(target, etc1s), is_pixel_target(target, etc1s), transcoder_format_name(target));
    return checked(ctx, [&](bu::err_text e) { return bu::build_transcode_slices(t, fn, slices, n_slices, n_inputs, p, d_out, out_bytes, e); });
}
