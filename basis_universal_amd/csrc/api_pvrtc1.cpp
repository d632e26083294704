// api_pvrtc1.cpp -- PVRTC1 4bpp RGB / RGBA behind the C ABI of libbasisu_hip.so, for both codecs: resident UASTC blocks, or resident ETC1S palettes + per-block
// indices, to a whole image in Morton order (pvrtc1_kernels.hip). A family of its own: the other transcoder families keep refusing targets 8 and 9.
#include "api_internal.h"
#include "etc1s_transcode_kernels.h"   // launch_etc1s_count_indices_past
#include "pvrtc1_kernels.h"

static const uint32_t kPvrtc1Rgb = 8, kPvrtc1Rgba = 9, kPvrtc1BlockBytes = 8;

static bool is_pow2(uint32_t v) { return v && !(v & (v - 1u)); }

// the refusals every entry shares, before any pointer is looked at: the target, then every decode flag, each by its name
static int pvrtc1_ok(bu_hip_context* ctx, const char* fn, uint32_t target, uint32_t decode_flags) {
    if (target != kPvrtc1Rgb && target != kPvrtc1Rgba) {
        set_error(ctx, "%s: target %u (%s) is not supported (supported: PVRTC1_4_RGB (8), PVRTC1_4_RGBA (9))", fn, target, transcoder_format_name(target));
        return 0;
    }
    if (decode_flags) {
        static const struct { uint32_t bit; const char* name; } flags[] = {
            { 2, "cDecodeFlagsPVRTCDecodeToNextPow2" }, { 4, "cDecodeFlagsTranscodeAlphaDataToOpaqueFormats" }, { 8, "cDecodeFlagsBC1ForbidThreeColorBlocks" },
            { 16, "cDecodeFlagsOutputHasAlphaIndices" }, { 32, "cDecodeFlagsHighQuality" }, { 64, "cDecodeFlagsNoETC1SChromaFiltering" },
            { 128, "cDecodeFlagsNoDeblockFiltering" }, { 512, "cDecodeFlagsForceDeblockFiltering" }, { 1024, "cDecodeFlagXUASTCLDRDisableFastBC7Transcoding" } };
        char names[400] = "";
        uint32_t unnamed = decode_flags;
        for (const auto& f : flags)
            if (decode_flags & f.bit) {
                snprintf(names + strlen(names), sizeof(names) - strlen(names), "%s%s", names[0] ? ", " : "", f.name);
                unnamed &= ~f.bit;
            }
        if (unnamed) snprintf(names + strlen(names), sizeof(names) - strlen(names), "%sunnamed bits 0x%x", names[0] ? ", " : "", unnamed);
        set_error(ctx, "%s: decode_flags 0x%x: %s not supported (the PVRTC1 entries take no decode flag)", fn, decode_flags, names);
        return 0;
    }
    return 1;
}

// one image's sizes: blocks that exist, pixels that fit them, powers of two throughout (the kernels wrap and interleave with masks)
static int pvrtc1_geometry(bu_hip_context* ctx, const char* who, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h) {
    if (!nbx || !nby) { set_error(ctx, "%s: zero blocks (%u x %u)", who, nbx, nby); return 0; }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry(who, nbx, nby, orig_w, orig_h, 0, 0, bu::kEachWay16384, &geo, e); })) return 0;
    if (!is_pow2(geo.width) || !is_pow2(geo.height) || !is_pow2(nbx) || !is_pow2(nby)) {
        set_error(ctx, "%s: %u x %u pixels in %u x %u blocks: PVRTC1 only supports power of 2 dimensions", who, geo.width, geo.height, nbx, nby);
        return 0;
    }
    return 1;
}

// one image through both launches; the count is read back behind one stream wait
static int pvrtc1_one_image(bu_hip_context* ctx, const char* fn, bu::pvrtc1_args& a, bu::pvrtc1_source source, uint32_t* out_invalid_blocks) {
    device_guard g(ctx->device);
    arena &counter = ctx->scratch[4], &words = ctx->scratch[5];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    BU_TRY(ctx, words.reserve((size_t)a.total_blocks * sizeof(uint32_t)));
    a.invalid = static_cast<uint32_t*>(counter.p);
    a.words = static_cast<uint32_t*>(words.p);
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_pvrtc1(ctx->stream, a, source));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

// the table forms: the whole-file transcoders' records under an 8-byte block target, every image a power of two, alpha slices in every record or in none
static int pvrtc1_table(bu_hip_context* ctx, const char* fn, bool etc1s, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target,
                        const void* d_out, size_t out_bytes, bu::slice_table& table, bool& any_alpha) {
    const bu::slice_policy p = bu::transcoder_slice_policy(etc1s, kPvrtc1BlockBytes, false, transcoder_format_name(target));
    if (!checked(ctx, [&](bu::err_text e) { return bu::build_transcode_slices(table, fn, slices, n_slices, n_inputs, p, d_out, out_bytes, e); })) return 0;
    uint32_t with_alpha = 0;
    for (uint32_t i = 0; i < n_slices; i++) {
        char who[96];
        snprintf(who, sizeof(who), "%s: slice %u", fn, i);
        if (!pvrtc1_geometry(ctx, who, slices[i].num_blocks_x, slices[i].num_blocks_y, slices[i].orig_width, slices[i].orig_height)) return 0;
        with_alpha += slices[i].alpha_first_block != BU_HIP_NO_ALPHA_SLICE;
    }
    if (with_alpha && with_alpha != n_slices) {
        set_error(ctx, "%s: %u of %u slices have an alpha slice: every image of a PVRTC1 call has one, or none has", fn, with_alpha, n_slices);
        return 0;
    }
    any_alpha = with_alpha != 0;
    return 1;
}

static int pvrtc1_run_table(bu_hip_context* ctx, const char* fn, const bu::slice_table& table, bu::pvrtc1_args& a, bu::pvrtc1_source source, uint32_t* out_invalid_per_slice) {
    device_guard g(ctx->device);
    arena& words = ctx->scratch[5];
    BU_TRY(ctx, words.reserve((size_t)table.total * sizeof(uint32_t)));
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    a.words = static_cast<uint32_t*>(words.p);
    a.invalid = d.counters;
    a.slices = static_cast<const bu_hip_transcode_slice*>(d.records);
    a.prefix = d.prefix;
    a.n_slices = table.n;
    a.total_blocks = table.total;
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_pvrtc1(ctx->stream, a, source));
    }
    return out_invalid_per_slice ? read_back(ctx, out_invalid_per_slice, d.counters, (size_t)table.n * sizeof(uint32_t)) : 1;
}

// the ETC1S one-image entries' checks; fills the launch arguments and the route
static int etc1s_pvrtc1_args(bu_hip_context* ctx, const char* fn, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                             const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                             uint32_t decode_flags, bu::pvrtc1_args& a, bu::pvrtc1_source& source) {
    if (!pvrtc1_ok(ctx, fn, target, decode_flags)) return 0;
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx || !d_out) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if ((d_a_ep_idx == nullptr) != (d_a_sel_idx == nullptr)) { set_error(ctx, "%s: an alpha slice needs both of its index arrays", fn); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "%s: palettes of %u endpoints and %u selectors (1..65535 each)", fn, n_ep, n_sel); return 0; }
    if (!pvrtc1_geometry(ctx, fn, nbx, nby, orig_w, orig_h)) return 0;
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) { set_error(ctx, "%s: the output must be 8-byte aligned", fn); return 0; }
    const bool alpha = target == kPvrtc1Rgba && d_a_ep_idx != nullptr;   // RGBA on an image without an alpha slice is the RGB route
    source = alpha ? bu::PVRTC1_FROM_ETC1S_RGBA : bu::PVRTC1_FROM_ETC1S_RGB;
    a = bu::pvrtc1_args{ static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                         static_cast<const uint16_t*>(d_sel_idx), alpha ? static_cast<const uint16_t*>(d_a_ep_idx) : nullptr,
                         alpha ? static_cast<const uint16_t*>(d_a_sel_idx) : nullptr, nullptr, nullptr, static_cast<uint8_t*>(d_out), nullptr, nullptr, nullptr, 0u, nbx * nby,
                         n_ep, n_sel, nbx, nby };
    return 1;
}

extern "C" {

size_t bu_hip_pvrtc1_output_bytes(uint32_t nbx, uint32_t nby) { return (size_t)nbx * nby * kPvrtc1BlockBytes; }

size_t bu_hip_pvrtc1_slice_extent(const bu_hip_transcode_slice* s, uint32_t target) {
    if (!s || (target != kPvrtc1Rgb && target != kPvrtc1Rgba)) return 0;
    return (size_t)s->num_blocks_x * s->num_blocks_y * kPvrtc1BlockBytes;
}

int bu_hip_k_transcode_uastc_pvrtc1(bu_hip_context* ctx, const void* d_blocks, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target,
                                    uint32_t decode_flags, void* d_out, uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_uastc_pvrtc1";
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    if (!pvrtc1_ok(ctx, fn, target, decode_flags)) return 0;
    if (!pvrtc1_geometry(ctx, fn, nbx, nby, orig_w, orig_h)) return 0;
    if (!d_blocks || !d_out) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    if ((reinterpret_cast<uintptr_t>(d_blocks) & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 7u)) {
        set_error(ctx, "%s: the blocks must be 16-byte aligned and the output 8-byte aligned", fn);
        return 0;
    }
    bu::pvrtc1_args a = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, static_cast<const uint4*>(d_blocks), nullptr, static_cast<uint8_t*>(d_out), nullptr, nullptr,
                          nullptr, 0u, nbx * nby, 0u, 0u, nbx, nby };
    return pvrtc1_one_image(ctx, fn, a, target == kPvrtc1Rgba ? bu::PVRTC1_FROM_UASTC_RGBA : bu::PVRTC1_FROM_UASTC_RGB, out_invalid_blocks);
}

int bu_hip_k_transcode_uastc_pvrtc1_images(bu_hip_context* ctx, const void* d_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
                                           uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_uastc_pvrtc1_images";
    if (!pvrtc1_ok(ctx, fn, target, decode_flags)) return 0;
    if (!d_blocks) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if (reinterpret_cast<uintptr_t>(d_blocks) & 15u) { set_error(ctx, "%s: the blocks are not 16-byte aligned", fn); return 0; }
    bu::slice_table table;
    bool any_alpha = false;
    if (!pvrtc1_table(ctx, fn, false, slices, n_slices, n_blocks, target, d_out, out_bytes, table, any_alpha)) return 0;
    bu::pvrtc1_args a = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, static_cast<const uint4*>(d_blocks), nullptr, static_cast<uint8_t*>(d_out), nullptr, nullptr,
                          nullptr, 0u, 0u, 0u, 0u, 0u, 0u };
    return pvrtc1_run_table(ctx, fn, table, a, target == kPvrtc1Rgba ? bu::PVRTC1_FROM_UASTC_RGBA : bu::PVRTC1_FROM_UASTC_RGB, out_invalid_per_slice);
}

int bu_hip_k_transcode_etc1s_pvrtc1_counted(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx,
                                            const void* d_sel_idx, const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h,
                                            uint32_t target, void* d_out, uint32_t decode_flags, uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    bu::pvrtc1_args a;
    bu::pvrtc1_source source;
    if (!etc1s_pvrtc1_args(ctx, "transcode_etc1s_pvrtc1", d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out,
                           decode_flags, a, source)) return 0;
    return pvrtc1_one_image(ctx, "transcode_etc1s_pvrtc1", a, source, out_invalid_blocks);
}

int bu_hip_k_transcode_etc1s_pvrtc1(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                    const void* d_a_ep_idx, const void* d_a_sel_idx, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t target, void* d_out,
                                    uint32_t decode_flags) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_etc1s_pvrtc1";
    bu::pvrtc1_args a;
    bu::pvrtc1_source source;
    if (!etc1s_pvrtc1_args(ctx, fn, d_ep_pal, n_ep, d_sel_pal, n_sel, d_ep_idx, d_sel_idx, d_a_ep_idx, d_a_sel_idx, nbx, nby, orig_w, orig_h, target, d_out, decode_flags, a,
                           source)) return 0;
    {   // the range check in front of the launches: a pass over the resident indices the route reads, one word back
        device_guard g(ctx->device);
        arena& counter = ctx->scratch[4];
        BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
        uint32_t* d_count = static_cast<uint32_t*>(counter.p);
        const uint32_t n = nbx * nby;
        {
            prof_scope ps(ctx, "etc1s_pvrtc1_check");
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.endpoint_idx, n, n_ep, d_count, true));
            BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.selector_idx, n, n_sel, d_count, false));
            if (a.alpha_endpoint_idx) {
                BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_endpoint_idx, n, n_ep, d_count, false));
                BU_TRY(ctx, bu::launch_etc1s_count_indices_past(ctx->stream, a.alpha_selector_idx, n, n_sel, d_count, false));
            }
        }
        uint32_t past = 0;
        if (!read_back(ctx, &past, d_count, sizeof(past))) return 0;
        if (past) { set_error(ctx, "%s: %u indices are past their palette (%u endpoints, %u selectors): nothing was transcoded", fn, past, n_ep, n_sel); return 0; }
    }
    uint32_t invalid = 0;
    if (!pvrtc1_one_image(ctx, fn, a, source, &invalid)) return 0;
    if (invalid) { set_error(ctx, "%s: %u blocks had an index past its palette", fn, invalid); return 0; }
    return 1;
}

int bu_hip_k_transcode_etc1s_pvrtc1_images(bu_hip_context* ctx, const void* d_ep_pal, uint32_t n_ep, const void* d_sel_pal, uint32_t n_sel, const void* d_ep_idx, const void* d_sel_idx,
                                           uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target, uint32_t decode_flags, void* d_out,
                                           size_t out_bytes, uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_etc1s_pvrtc1_images";
    if (!pvrtc1_ok(ctx, fn, target, decode_flags)) return 0;
    if (!d_ep_pal || !d_sel_pal || !d_ep_idx || !d_sel_idx) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if (!n_ep || !n_sel || n_ep > 65535u || n_sel > 65535u) { set_error(ctx, "%s: palettes of %u endpoints and %u selectors (1..65535 each)", fn, n_ep, n_sel); return 0; }
    bu::slice_table table;
    bool any_alpha = false;
    if (!pvrtc1_table(ctx, fn, true, slices, n_slices, n_indices, target, d_out, out_bytes, table, any_alpha)) return 0;
    bu::pvrtc1_args a = { static_cast<const uint32_t*>(d_ep_pal), static_cast<const uint32_t*>(d_sel_pal), static_cast<const uint16_t*>(d_ep_idx),
                          static_cast<const uint16_t*>(d_sel_idx), nullptr, nullptr, nullptr, nullptr, static_cast<uint8_t*>(d_out), nullptr, nullptr, nullptr, 0u, 0u, n_ep, n_sel,
                          0u, 0u };
    return pvrtc1_run_table(ctx, fn, table, a, target == kPvrtc1Rgba && any_alpha ? bu::PVRTC1_FROM_ETC1S_RGBA : bu::PVRTC1_FROM_ETC1S_RGB, out_invalid_per_slice);
}

}  // extern "C"
