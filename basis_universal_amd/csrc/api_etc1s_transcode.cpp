// api_etc1s_transcode.cpp -- the ETC1S transcoder behind the C ABI of libbasisu_hip.so: palettes + per-block indices (host/etc1s_decode.cpp's output, resident) -> texture.
#include "api_internal.h"
#include "etc1s_transcode_kernels.h"

static const char* const kEtc1sTargets = "ETC1_RGB (0), BC1_RGB (2), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16)";
static const char* const kEtc1sTextureTargets = "ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16)";
static const char* const kEtc1sBlockFormatTargets = "ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), ASTC_4x4_RGBA (10), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16), "
                                                    "ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21)";
static const char* const kEtc1sVendorFormatTargets = "ETC1_RGB (0), ETC2_RGBA (1), BC1_RGB (2), BC7_RGBA (6), ASTC_4x4_RGBA (10), ATC_RGB (11), RGBA32 (13), RGB565 (14), BGR565 (15), "
                                                     "RGBA4444 (16), FXT1_RGB (17), PVRTC2_4_RGB (18), PVRTC2_4_RGBA (19), ETC2_EAC_R11 (20), ETC2_EAC_RG11 (21)";
static const uint32_t kNoChromaFiltering = 64;   // cDecodeFlagsNoETC1SChromaFiltering, the one flag of the bu_hip_k_transcode_etc1s_image* entries

// Which entry family a call came through. The first (bu_hip_k_transcode_etc1s*) has six targets and no flags; the second (bu_hip_k_transcode_etc1s_image*) adds the
// 16-byte targets and decode_flags; the third (bu_hip_k_transcode_etc1s_block_format*) adds ASTC 4x4 and EAC R11 / RG11; the fourth (bu_hip_k_transcode_etc1s_vendor_format*)
// adds ATC RGB, FXT1 and PVRTC2 RGB / RGBA. All run the same code below: the family decides the target list, the flags, the name in a refusal and, the fourth, why a target
// it names is missing.
struct etc1s_family { const char* fn; const char* targets; uint32_t (*unit_bytes)(uint32_t target); const char* (*why_not)(uint32_t target); };
// what the fourth family says of the targets it refuses for a reason
static const char* vendor_format_why_not(uint32_t target) {
    if (target == 3 || target == 4 || target == 5) return ": it needs the ETC1S -> BC4 look-up, which could not be restated as a search";
    if (target == 12) return ": its first half is a BC4 block, and the ETC1S -> BC4 look-up could not be restated as a search";
    return "";
}
static const etc1s_family kFirstFamily = { "transcode_etc1s", kEtc1sTargets, bu::etc1s_transcode_unit_bytes, nullptr },
                          kImageFamily = { "transcode_etc1s_image", kEtc1sTextureTargets, bu::etc1s_texture_unit_bytes, nullptr },
                          kBlockFormatFamily = { "transcode_etc1s_block_format", kEtc1sBlockFormatTargets, bu::etc1s_block_format_unit_bytes, nullptr },
                          kVendorFormatFamily = { "transcode_etc1s_vendor_format", kEtc1sVendorFormatTargets, bu::etc1s_vendor_format_unit_bytes, vendor_format_why_not };

static uint32_t family_unit_bytes(const etc1s_family& f, uint32_t target) { return f.unit_bytes(target); }
static bool reads_alpha(uint32_t target) {
    return target == bu::ETF_RGBA32 || target == bu::ETF_RGBA4444 || target == bu::ETF_ETC2_RGBA || target == bu::ETF_BC7_RGBA || target == bu::ETF_ASTC_4x4_RGBA ||
           target == bu::ETF_ETC2_EAC_RG11 || target == bu::ETF_PVRTC2_4_RGBA;
}
// the target and the flags of a call; the refusal names what is wrong
static int etc1s_target_ok(bu_hip_context* ctx, const etc1s_family& f, uint32_t target, uint32_t decode_flags) {
    if (!family_unit_bytes(f, target)) {
        set_error(ctx, "%s: target %u (%s) is not supported%s (supported: %s)", f.fn, target, transcoder_format_name(target), f.why_not ? f.why_not(target) : "", f.targets);
        return 0;
    }
    if (decode_flags & ~kNoChromaFiltering) {
        set_error(ctx, "%s: decode_flags 0x%x: bits 0x%x are not supported (supported: 64, cDecodeFlagsNoETC1SChromaFiltering)", f.fn, decode_flags, decode_flags & ~kNoChromaFiltering);
        return 0;
    }
    return 1;
}

// the checks both entry points share; fills the launch arguments
static int etc1s_transcode_args_from(bu_hip_context* ctx, const etc1s_family& f, uint32_t decode_flags, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                     const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                     uint32_t pitch_px, uint32_t rows_px, bu::etc1s_transcode_args& a) {
    if (!etc1s_target_ok(ctx, f, target, decode_flags)) return 0;
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx || !d_out) { set_error(ctx, "%s: null device pointer", f.fn); return 0; }
    if ((d_a_ep_idx == nullptr) != (d_a_sel_idx == nullptr)) { set_error(ctx, "%s: an alpha slice needs both of its index arrays", f.fn); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "%s: palettes of %u endpoints and %u selectors (1..65535 each)", f.fn, n_ep, n_sel); return 0; }
    if (family_unit_bytes(f, target) == 16 && (reinterpret_cast<uintptr_t>(d_out) & 15u)) { set_error(ctx, "%s: the output of a 16-byte target must be 16-byte aligned", f.fn); return 0; }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry(f.fn, nbx, nby, orig_w, orig_h, pitch_px, rows_px, bu::kEachWay16384, &geo, e); })) return 0;
    a = bu::etc1s_transcode_args{ static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                                  static_cast<const uint16_t*>(d_sel_idx), static_cast<const uint16_t*>(d_a_ep_idx), static_cast<const uint16_t*>(d_a_sel_idx), d_out, nullptr, nullptr,
                                  nullptr, n_ep, n_sel, geo };
    return 1;
}

// the ETC1S -> BC1 endpoint tables of this context: built on its stream by the first BC1 transcode, resident until the context goes
static int ensure_bc1_tables(bu_hip_context* ctx) {
    if (ctx->etc1s_bc1_tables.p) return 1;
    BU_TRY(ctx, ctx->etc1s_bc1_tables.reserve(2 * bu::kBc1TableEntries * sizeof(uint32_t)));
    hipError_t e = bu::launch_etc1s_build_bc1_tables(ctx->stream, static_cast<uint32_t*>(ctx->etc1s_bc1_tables.p));
    if (e != hipSuccess) { ctx->etc1s_bc1_tables.release(); set_error(ctx, "etc1s_build_bc1_tables: %s", hipGetErrorString(e)); return 0; }
    return 1;
}

// the ETC1S -> BC7 colour look-up and the encoder's midpoints, the same way: built by the first BC7 transcode, released with the context
static int ensure_bc7_tables(bu_hip_context* ctx) {
    if (ctx->etc1s_bc7_tables.p) return 1;
    BU_TRY(ctx, ctx->etc1s_bc7_tables.reserve(bu::kEtc1sBc7TableWords * sizeof(uint32_t)));
    hipError_t e = bu::launch_etc1s_build_bc7_tables(ctx->stream, static_cast<uint32_t*>(ctx->etc1s_bc7_tables.p));
    if (e != hipSuccess) { ctx->etc1s_bc7_tables.release(); set_error(ctx, "etc1s_build_bc7_tables: %s", hipGetErrorString(e)); return 0; }
    return 1;
}
// the two ETC1S -> ASTC look-ups and the unquantised endpoint values, the same way: built by the first ASTC transcode
static int ensure_astc_tables(bu_hip_context* ctx) {
    if (ctx->etc1s_astc_tables.p) return 1;
    BU_TRY(ctx, ctx->etc1s_astc_tables.reserve(bu::kEtc1sAstcTableWords * sizeof(uint32_t)));
    hipError_t e = bu::launch_etc1s_build_astc_tables(ctx->stream, static_cast<uint32_t*>(ctx->etc1s_astc_tables.p));
    if (e != hipSuccess) { ctx->etc1s_astc_tables.release(); set_error(ctx, "etc1s_build_astc_tables: %s", hipGetErrorString(e)); return 0; }
    return 1;
}
// the three ETC1S -> ATC / PVRTC2 look-ups, the same way: built by the first ATC RGB or PVRTC2 RGB / RGBA transcode
static int ensure_atc_tables(bu_hip_context* ctx) {
    if (ctx->etc1s_atc_tables.p) return 1;
    BU_TRY(ctx, ctx->etc1s_atc_tables.reserve(bu::kEtc1sAtcTableWords * sizeof(uint32_t)));
    hipError_t e = bu::launch_etc1s_build_atc_tables(ctx->stream, static_cast<uint32_t*>(ctx->etc1s_atc_tables.p));
    if (e != hipSuccess) { ctx->etc1s_atc_tables.release(); set_error(ctx, "etc1s_build_atc_tables: %s", hipGetErrorString(e)); return 0; }
    return 1;
}
// only what the target needs; FXT1 goes through BC1's tables
static int ensure_target_tables(bu_hip_context* ctx, uint32_t target, const uint32_t*& bc1, const uint32_t*& bc7, const uint32_t*& astc, const uint32_t*& atc) {
    if (target == bu::ETF_ATC_RGB || target == bu::ETF_PVRTC2_4_RGB || target == bu::ETF_PVRTC2_4_RGBA) {
        if (!ensure_atc_tables(ctx)) return 0;
        atc = static_cast<const uint32_t*>(ctx->etc1s_atc_tables.p);
    }
    if (target == bu::ETF_ASTC_4x4_RGBA) {
        if (!ensure_astc_tables(ctx)) return 0;
        astc = static_cast<const uint32_t*>(ctx->etc1s_astc_tables.p);
    }
    if (target == bu::ETF_BC1_RGB || target == bu::ETF_FXT1_RGB) {
        if (!ensure_bc1_tables(ctx)) return 0;
        bc1 = static_cast<const uint32_t*>(ctx->etc1s_bc1_tables.p);
    }
    if (target == bu::ETF_BC7_RGBA) {
        if (!ensure_bc7_tables(ctx)) return 0;
        bc7 = static_cast<const uint32_t*>(ctx->etc1s_bc7_tables.p);
    }
    return 1;
}

// one image, counted: both families' *_counted entries
static int transcode_image_counted(bu_hip_context* ctx, const etc1s_family& f, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                                   const void* d_sel_idx, const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target,
                                   void* d_out, uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags, uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    bu::etc1s_transcode_args a;
    if (!etc1s_transcode_args_from(ctx, f, decode_flags, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, a)) return 0;
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    a.invalid = static_cast<uint32_t*>(counter.p);
    const uint32_t* atc = nullptr;
    if (!ensure_target_tables(ctx, target, a.bc1_endpoints, a.bc7_tables, a.astc_tables, atc)) return 0;
    {
        prof_scope ps(ctx, "etc1s_transcode");
        BU_TRY(ctx, bu::launch_transcode_etc1s_any_target(ctx->stream, a, atc, target, !(decode_flags & kNoChromaFiltering)));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

// one image behind a range check of every index the target reads: both families' plain entries
static int transcode_image_checked(bu_hip_context* ctx, const etc1s_family& f, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                                   const void* d_sel_idx, const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target,
                                   void* d_out, uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags) {
    if (!ctx) return 0;
    bu::etc1s_transcode_args a;
    if (!etc1s_transcode_args_from(ctx, f, decode_flags, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, a)) return 0;
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    uint32_t* d_count = static_cast<uint32_t*>(counter.p);
    const uint32_t n = nbx * nby;
    // the indices are resident, so the range check that has to come before the launch is a pass over them on the device: 2-4 bytes per block read, one word back
    {
        prof_scope ps(ctx, "etc1s_transcode_check");
        BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.endpoint_idx, n, n_ep, d_count, true));
        BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.selector_idx, n, n_sel, d_count, false));
        if (a.alpha_endpoint_idx && reads_alpha(target)) {
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_endpoint_idx, n, n_ep, d_count, false));
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_selector_idx, n, n_sel, d_count, false));
        }
    }
    uint32_t past = 0;
    if (!read_back(ctx, &past, d_count, sizeof(past))) return 0;
    if (past) { set_error(ctx, "%s: %u indices are past their palette (%u endpoints, %u selectors): nothing was transcoded", f.fn, past, n_ep, n_sel); return 0; }
    uint32_t invalid = 0;
    if (!transcode_image_counted(ctx, f, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px, rows_px, decode_flags,
                                 &invalid)) return 0;
    if (invalid) { set_error(ctx, "%s: %u blocks had an index past its palette", f.fn, invalid); return 0; }
    return 1;
}

// every image of a file in one launch: the table's checks and pack are tile_geometry_check.h's behind etc1s_slices_check, upload and read-back api_internal.h's
static int transcode_images(bu_hip_context* ctx, const etc1s_family& f, const char* fn, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                            const void* d_sel_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, uint32_t decode_flags, void* d_out,
                            size_t out_bytes, uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    if (!etc1s_target_ok(ctx, f, target, decode_flags)) return 0;
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "%s: palettes of %u endpoints and %u selectors (1..65535 each)", fn, n_ep, n_sel); return 0; }
    bu::slice_table table;
    if (!etc1s_slices_check(ctx, table, fn, slices, n_slices, n_indices, target, family_unit_bytes(f, target), d_out, out_bytes, target == bu::ETF_FXT1_RGB)) return 0;
    device_guard g(ctx->device);
    const uint32_t *bc1 = nullptr, *bc7 = nullptr, *astc = nullptr, *atc = nullptr;
    if (!ensure_target_tables(ctx, target, bc1, bc7, astc, atc)) return 0;
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    const bu::etc1s_transcode_slices_args a = { static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                                                static_cast<const uint16_t*>(d_sel_idx), static_cast<uint8_t*>(d_out), d.counters, bc1, bc7,
                                                static_cast<const bu_hip_transcode_slice*>(d.records), d.prefix, n_ep, n_sel, table.n, table.total, astc };
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_etc1s_any_target_slices(ctx->stream, a, atc, target, !(decode_flags & kNoChromaFiltering)));
    }
    return out_invalid_per_slice ? read_back(ctx, out_invalid_per_slice, d.counters, (size_t)table.n * sizeof(uint32_t)) : 1;
}

extern "C" {

size_t bu_hip_etc1s_transcode_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, uint32_t pitch_px, uint32_t rows_px) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_w, orig_h, pitch_px, rows_px }, bu::etc1s_transcode_unit_bytes(target),
                                   bu::etc1s_transcode_is_pixel_target(target));
}

int bu_hip_etc1s_bc1_endpoint_tables(bu_hip_context* ctx, uint32_t* h_out5, uint32_t* h_out6) {
    if (!ctx || !h_out5 || !h_out6) { if (ctx) set_error(ctx, "etc1s_bc1_endpoint_tables: null pointer"); return 0; }
    device_guard g(ctx->device);
    if (!ensure_bc1_tables(ctx)) return 0;
    const uint32_t* d = static_cast<const uint32_t*>(ctx->etc1s_bc1_tables.p);
    if (!fetch(ctx, h_out5, d, bu::kBc1TableEntries * sizeof(uint32_t)) || !fetch(ctx, h_out6, d + bu::kBc1TableEntries, bu::kBc1TableEntries * sizeof(uint32_t))) return 0;
    return 1;
}

int bu_hip_k_transcode_etc1s_counted(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                     const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                     uint32_t pitch_px, uint32_t rows_px, uint32_t* out_invalid_blocks) {
    return transcode_image_counted(ctx, kFirstFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, 0, out_invalid_blocks);
}

int bu_hip_k_transcode_etc1s(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                             const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                             uint32_t pitch_px, uint32_t rows_px) {
    return transcode_image_checked(ctx, kFirstFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, 0);
}

int bu_hip_k_transcode_etc1s_slices(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                    uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, void* d_out, size_t out_bytes,
                                    uint32_t* out_invalid_per_slice) {
    return transcode_images(ctx, kFirstFamily, "transcode_etc1s_slices", d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, n_indices, slices, n_slices, target, 0, d_out, out_bytes,
                            out_invalid_per_slice);
}

// ---- the second family: the first one's arguments plus decode_flags, all eight targets

size_t bu_hip_etc1s_image_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, uint32_t pitch_px, uint32_t rows_px) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_w, orig_h, pitch_px, rows_px }, bu::etc1s_texture_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target));
}

int bu_hip_etc1s_bc7_color_table(bu_hip_context* ctx, uint32_t* h_out, uint32_t* h_midpoints) {
    if (!ctx || !h_out || !h_midpoints) { if (ctx) set_error(ctx, "etc1s_bc7_color_table: null pointer"); return 0; }
    device_guard g(ctx->device);
    if (!ensure_bc7_tables(ctx)) return 0;
    const uint32_t* d = static_cast<const uint32_t*>(ctx->etc1s_bc7_tables.p);
    const size_t n = bu::kEtc1sBc7TableWords - 128;
    return fetch(ctx, h_out, d, n * sizeof(uint32_t)) && fetch(ctx, h_midpoints, d + n, 128 * sizeof(uint32_t)) ? 1 : 0;
}

int bu_hip_k_bc7_mode5_tiles(bu_hip_context* ctx, const void* d_tiles, uint32_t n_tiles, void* d_out) {
    if (!ctx) return 0;
    if (!d_tiles || !d_out) { set_error(ctx, "bc7_mode5_tiles: null device pointer"); return 0; }
    if ((reinterpret_cast<uintptr_t>(d_tiles) | reinterpret_cast<uintptr_t>(d_out)) & 15u) { set_error(ctx, "bc7_mode5_tiles: the tiles and the output must be 16-byte aligned"); return 0; }
    if (n_tiles > (1u << 30)) { set_error(ctx, "bc7_mode5_tiles: %u tiles is too many (at most 2^30)", n_tiles); return 0; }
    if (!n_tiles) return 1;
    device_guard g(ctx->device);
    if (!ensure_bc7_tables(ctx)) return 0;
    prof_scope ps(ctx, "bc7_mode5_tiles");
    BU_TRY(ctx, bu::launch_bc7_mode5_tiles(ctx->stream, d_tiles, n_tiles, d_out, static_cast<const uint32_t*>(ctx->etc1s_bc7_tables.p)));
    return 1;
}

int bu_hip_k_transcode_etc1s_image_counted(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                           const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                           uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags, uint32_t* out_invalid_blocks) {
    return transcode_image_counted(ctx, kImageFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, decode_flags, out_invalid_blocks);
}

int bu_hip_k_transcode_etc1s_image(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                   const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                   uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags) {
    return transcode_image_checked(ctx, kImageFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px,
                                   rows_px, decode_flags);
}

int bu_hip_k_transcode_etc1s_images(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                    uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, uint32_t decode_flags, void* d_out, size_t out_bytes,
                                    uint32_t* out_invalid_per_slice) {
    return transcode_images(ctx, kImageFamily, "transcode_etc1s_images", d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, n_indices, slices, n_slices, target, decode_flags, d_out,
                            out_bytes, out_invalid_per_slice);
}

// ---- the third family: the second one's arguments, all eleven targets

size_t bu_hip_etc1s_block_format_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, uint32_t pitch_px, uint32_t rows_px) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_w, orig_h, pitch_px, rows_px }, bu::etc1s_block_format_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target));
}

int bu_hip_etc1s_astc_tables(bu_hip_context* ctx, uint32_t* h_out_0_47, uint32_t* h_out_0_255, uint32_t* h_unquant48) {
    if (!ctx || !h_out_0_47 || !h_out_0_255 || !h_unquant48) { if (ctx) set_error(ctx, "etc1s_astc_tables: null pointer"); return 0; }
    device_guard g(ctx->device);
    if (!ensure_astc_tables(ctx)) return 0;
    const uint32_t* d = static_cast<const uint32_t*>(ctx->etc1s_astc_tables.p);
    const size_t n = (bu::kEtc1sAstcTableWords - 48) / 2;
    return fetch(ctx, h_out_0_47, d, n * sizeof(uint32_t)) && fetch(ctx, h_out_0_255, d + n, n * sizeof(uint32_t)) && fetch(ctx, h_unquant48, d + 2 * n, 48 * sizeof(uint32_t)) ? 1 : 0;
}

int bu_hip_k_transcode_etc1s_block_format_counted(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                                                  const void* d_sel_idx, const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h,
                                                  uint32_t target, void* d_out, uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags, uint32_t* out_invalid_blocks) {
    return transcode_image_counted(ctx, kBlockFormatFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out,
                                   pitch_px, rows_px, decode_flags, out_invalid_blocks);
}

int bu_hip_k_transcode_etc1s_block_format(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                          const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                          uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags) {
    return transcode_image_checked(ctx, kBlockFormatFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out,
                                   pitch_px, rows_px, decode_flags);
}

int bu_hip_k_transcode_etc1s_block_formats(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                           uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, uint32_t decode_flags, void* d_out,
                                           size_t out_bytes, uint32_t* out_invalid_per_slice) {
    return transcode_images(ctx, kBlockFormatFamily, "transcode_etc1s_block_formats", d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, n_indices, slices, n_slices, target,
                            decode_flags, d_out, out_bytes, out_invalid_per_slice);
}

// ---- the fourth family: the third one's arguments and targets, and ATC RGB, FXT1, PVRTC2 RGB and PVRTC2 RGBA

size_t bu_hip_etc1s_vendor_format_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, uint32_t pitch_px, uint32_t rows_px) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_w, orig_h, pitch_px, rows_px }, bu::etc1s_vendor_format_unit_bytes(target), bu::etc1s_transcode_is_pixel_target(target),
                                   target == bu::ETF_FXT1_RGB);
}

int bu_hip_etc1s_atc_tables(bu_hip_context* ctx, uint32_t* h_out_55, uint32_t* h_out_56, uint32_t* h_out_45) {
    if (!ctx || !h_out_55 || !h_out_56 || !h_out_45) { if (ctx) set_error(ctx, "etc1s_atc_tables: null pointer"); return 0; }
    device_guard g(ctx->device);
    if (!ensure_atc_tables(ctx)) return 0;
    const uint32_t* d = static_cast<const uint32_t*>(ctx->etc1s_atc_tables.p);
    const size_t n = bu::kEtc1sAtcTableWords / 3;
    return fetch(ctx, h_out_55, d, n * sizeof(uint32_t)) && fetch(ctx, h_out_56, d + n, n * sizeof(uint32_t)) && fetch(ctx, h_out_45, d + 2 * n, n * sizeof(uint32_t)) ? 1 : 0;
}

int bu_hip_k_transcode_etc1s_vendor_format_counted(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                                                   const void* d_sel_idx, const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h,
                                                   uint32_t target, void* d_out, uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags, uint32_t* out_invalid_blocks) {
    return transcode_image_counted(ctx, kVendorFormatFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out,
                                   pitch_px, rows_px, decode_flags, out_invalid_blocks);
}

int bu_hip_k_transcode_etc1s_vendor_format(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                           const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                           uint32_t pitch_px, uint32_t rows_px, uint32_t decode_flags) {
    return transcode_image_checked(ctx, kVendorFormatFamily, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out,
                                   pitch_px, rows_px, decode_flags);
}

int bu_hip_k_transcode_etc1s_vendor_formats(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                            uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, uint32_t decode_flags, void* d_out,
                                            size_t out_bytes, uint32_t* out_invalid_per_slice) {
    return transcode_images(ctx, kVendorFormatFamily, "transcode_etc1s_vendor_formats", d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, n_indices, slices, n_slices, target,
                            decode_flags, d_out, out_bytes, out_invalid_per_slice);
}

} // extern "C"
