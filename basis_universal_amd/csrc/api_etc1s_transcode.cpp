// api_etc1s_transcode.cpp -- the ETC1S transcoder behind the C ABI of libbasisu_hip.so: palettes + per-block indices (host/etc1s_decode.cpp's output, resident) -> texture.
#include "api_internal.h"
#include "etc1s_transcode_kernels.h"

static const char* const kEtc1sTargets = "ETC1_RGB (0), BC1_RGB (2), RGBA32 (13), RGB565 (14), BGR565 (15), RGBA4444 (16)";

// the checks both entry points share; fills the launch arguments
static int etc1s_transcode_args_from(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                     const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                     uint32_t pitch_px, uint32_t rows_px, bu::etc1s_transcode_args& a) {
    if (!bu::etc1s_transcode_unit_bytes(target)) {
        set_error(ctx, "transcode_etc1s: target %u (%s) is not supported (supported: %s)", target, transcoder_format_name(target), kEtc1sTargets);
        return 0;
    }
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx || !d_out) { set_error(ctx, "transcode_etc1s: null device pointer"); return 0; }
    if ((d_a_ep_idx == nullptr) != (d_a_sel_idx == nullptr)) { set_error(ctx, "transcode_etc1s: an alpha slice needs both of its index arrays"); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "transcode_etc1s: palettes of %u endpoints and %u selectors (1..65535 each)", n_ep, n_sel); return 0; }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry("transcode_etc1s", nbx, nby, orig_w, orig_h, pitch_px, rows_px, bu::kEachWay16384, &geo, e); })) return 0;
    a = bu::etc1s_transcode_args{ static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                                  static_cast<const uint16_t*>(d_sel_idx), static_cast<const uint16_t*>(d_a_ep_idx), static_cast<const uint16_t*>(d_a_sel_idx), d_out, nullptr, nullptr,
                                  n_ep, n_sel, geo };
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
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    bu::etc1s_transcode_args a;
    if (!etc1s_transcode_args_from(ctx, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px, rows_px, a)) return 0;
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    a.invalid = static_cast<uint32_t*>(counter.p);
    if (target == bu::ETF_BC1_RGB) {
        if (!ensure_bc1_tables(ctx)) return 0;
        a.bc1_endpoints = static_cast<const uint32_t*>(ctx->etc1s_bc1_tables.p);
    }
    {
        prof_scope ps(ctx, "etc1s_transcode");
        BU_TRY(ctx, bu::launch_transcode_etc1s(ctx->stream, a, target));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

int bu_hip_k_transcode_etc1s(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                             const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                             uint32_t pitch_px, uint32_t rows_px) {
    if (!ctx) return 0;
    bu::etc1s_transcode_args a;
    if (!etc1s_transcode_args_from(ctx, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px, rows_px, a)) return 0;
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
        const bool alpha_read = a.alpha_endpoint_idx && (target == bu::ETF_RGBA32 || target == bu::ETF_RGBA4444);
        if (alpha_read) {
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_endpoint_idx, n, n_ep, d_count, false));
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_selector_idx, n, n_sel, d_count, false));
        }
    }
    uint32_t past = 0;
    if (!read_back(ctx, &past, d_count, sizeof(past))) return 0;
    if (past) { set_error(ctx, "transcode_etc1s: %u indices are past their palette (%u endpoints, %u selectors): nothing was transcoded", past, n_ep, n_sel); return 0; }
    uint32_t invalid = 0;
    if (!bu_hip_k_transcode_etc1s_counted(ctx, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, pitch_px, rows_px,
                                          &invalid)) return 0;
    if (invalid) { set_error(ctx, "transcode_etc1s: %u blocks had an index past its palette", invalid); return 0; }
    return 1;
}

// every image of a file in one launch: the table's checks and pack are tile_geometry_check.h's behind transcode_slices_check, upload and read-back api_internal.h's
int bu_hip_k_transcode_etc1s_slices(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                    uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, void* d_out, size_t out_bytes,
                                    uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_etc1s_slices";
    if (!bu::etc1s_transcode_unit_bytes(target)) {
        set_error(ctx, "transcode_etc1s: target %u (%s) is not supported (supported: %s)", target, transcoder_format_name(target), kEtc1sTargets);
        return 0;
    }
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "%s: palettes of %u endpoints and %u selectors (1..65535 each)", fn, n_ep, n_sel); return 0; }
    bu::slice_table table;
    if (!transcode_slices_check(ctx, table, fn, slices, n_slices, n_indices, target, true, d_out, out_bytes)) return 0;
    device_guard g(ctx->device);
    const uint32_t* bc1 = nullptr;
    if (target == bu::ETF_BC1_RGB) {
        if (!ensure_bc1_tables(ctx)) return 0;
        bc1 = static_cast<const uint32_t*>(ctx->etc1s_bc1_tables.p);
    }
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    const bu::etc1s_transcode_slices_args a = { static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                                                static_cast<const uint16_t*>(d_sel_idx), static_cast<uint8_t*>(d_out), d.counters, bc1,
                                                static_cast<const bu_hip_transcode_slice*>(d.records), d.prefix, n_ep, n_sel, table.n, table.total };
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_etc1s_slices(ctx->stream, a, target));
    }
    return out_invalid_per_slice ? read_back(ctx, out_invalid_per_slice, d.counters, (size_t)table.n * sizeof(uint32_t)) : 1;
}

} // extern "C"
