// api_uastc.cpp -- UASTC behind the C ABI of libbasisu_hip.so (rows a16-a19): encode (device-resident and blocking), transcode, RDO, the pipeline of images in flight.
#include "api_internal.h"
#include "uastc_kernels.h"
#include "uastc_rdo_strips.h"
#include "uastc_transcode_kernels.h"

// ---------------------------------------------------------------- UASTC (+ RDO) over a stream of images: several in flight (BASELINE configs[4])
//
// uastc_rdo's walk is a serial chain per strip (uastc_enc.cpp:3824-4100): one workgroup per strip, ~3 us per block, so the strips of one batch of images occupy a
// fraction of the chip for ~20 ms whatever the batch holds (96 strips of the Kodak batch: 96 of 256 CUs). Nothing in one batch can fill the rest -- the next batch can:
// its encode / prepare kernels (and the previous batch's finish) run on the idle CUs while this batch's strips walk. The pipeline owns `lanes` private contexts (stream +
// workspaces each); a submission is ENQUEUED on the next lane without any host synchronisation -- the finish kernel is launched for the longest list a strip can have
// instead of waiting for the walk to learn the real one -- and completes behind an event. Results are those of bu_hip_k_encode_uastc_blocks + bu_hip_k_uastc_rdo.
struct bu_uastc_pipeline {
    struct lane { bu_hip_context* ctx = nullptr; hipEvent_t done = nullptr, input = nullptr; uint32_t* stats = nullptr; bool busy = false, with_rdo = false; uint64_t ticket = 0; uint32_t strips = 0; };
    bu_hip_context* parent = nullptr;
    std::vector<lane> lanes;
    uint64_t next_ticket = 1;
    size_t ws_bytes = 0;   // what create sized every lane's workspace for: submit's limit (a parked lane context may come back with a larger arena; the limit does not move with it)
};

extern "C" {
// ---------------------------------------------------------------- UASTC (rows a16-a19)

size_t bu_hip_uastc_workspace_bytes(uint32_t n_blocks, uint32_t flags) { return bu::uastc_workspace_bytes(n_blocks, flags); }
size_t bu_hip_uastc_rdo_workspace_bytes(uint32_t n_blocks, uint32_t total_jobs) { return bu::uastc_rdo_workspace_bytes(n_blocks, total_jobs); }

int bu_hip_k_encode_uastc_blocks(bu_hip_context* ctx, const void* d_px, uint32_t n_blocks, uint32_t flags, void* d_out) {
    if (!ctx) return 0;
    if (!d_px || !d_out) { set_error(ctx, "encode_uastc: null device pointer"); return 0; }
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[5];
    BU_TRY(ctx, ws.reserve(bu::uastc_workspace_bytes(n_blocks, flags)));
    static const char* const names[4] = { "uastc_classify", "uastc_candidates", "uastc_score", "uastc_finish" };
    for (int phase = 0; phase < 4; phase++) {
        prof_scope ps(ctx, names[phase]);
        BU_TRY(ctx, bu::launch_uastc_phase(ctx->stream, phase, d_px, n_blocks, flags, ws.p, d_out));
    }
    return 1;
}

int bu_hip_encode_uastc_blocks(bu_hip_context* ctx, bu_uastc_block* out, uint32_t flags) {
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    arena& o = ctx->scratch[0];
    BU_TRY(ctx, o.reserve((size_t)n * 16));
    if (!bu_hip_k_encode_uastc_blocks(ctx, ctx->d_pixel_blocks, n, flags, o.p)) return 0;
    if (!fetch(ctx, out, o.p, (size_t)n * 16)) return 0;
    return 1;
}

// ---------------------------------------------------------------- UASTC transcode (uastc_transcode_kernels.hip)

static const char* const kUastcTargetRefused = "transcode_uastc: target %u is not supported (RGBA32, ASTC 4x4, BC1, BC3, BC4, BC5, BC7 are)";   // both entries' text

size_t bu_hip_transcode_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_width, uint32_t orig_height, uint32_t target) {
    return bu::transcode_output_bytes(nbx, nby, orig_width, orig_height, target);
}

int bu_hip_k_transcode_uastc(bu_hip_context* ctx, const void* d_blocks, uint32_t nbx, uint32_t nby, uint32_t orig_width, uint32_t orig_height, uint32_t target,
                             uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels,
                             uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    if (!bu::transcode_output_bytes(1, 1, 0, 0, target)) { set_error(ctx, kUastcTargetRefused, target); return 0; }
    if (!d_blocks || !d_out) { set_error(ctx, "transcode_uastc: null device pointer"); return 0; }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) {
            return bu::resolve_geometry("transcode_uastc", nbx, nby, orig_width, orig_height, out_row_pitch_pixels, out_rows_pixels, bu::kUastcOneImage, &geo, e);
        })) return 0;
    if (channel0 > 3 || channel1 > 3) { set_error(ctx, "transcode_uastc: channel out of range"); return 0; }
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    {
        prof_scope ps(ctx, "uastc_transcode");
        BU_TRY(ctx, bu::launch_transcode_uastc(ctx->stream, d_blocks, geo, target, (decode_flags & 32u) != 0 /* cDecodeFlagsHighQuality */,
                                               channel0 < 0 ? 0u : (uint32_t)channel0, channel1 < 0 ? 3u : (uint32_t)channel1, d_out, static_cast<uint32_t*>(counter.p)));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

// every image of a file in one launch: the table's checks and pack are tile_geometry_check.h's behind transcode_slices_check, upload and read-back api_internal.h's
int bu_hip_k_transcode_uastc_slices(bu_hip_context* ctx, const void* d_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
                                    uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_uastc_slices";
    if (!bu::transcode_output_bytes(1, 1, 0, 0, target)) { set_error(ctx, kUastcTargetRefused, target); return 0; }
    if (!d_blocks) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if ((uintptr_t)d_blocks & 15u) { set_error(ctx, "%s: the blocks are not 16-byte aligned", fn); return 0; }
    if (channel0 > 3 || channel1 > 3) { set_error(ctx, "%s: channel out of range", fn); return 0; }
    bu::slice_table table;
    if (!transcode_slices_check(ctx, table, fn, slices, n_slices, n_blocks, target, false, d_out, out_bytes)) return 0;
    device_guard g(ctx->device);
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_uastc_slices(ctx->stream, d_blocks, static_cast<const bu_hip_transcode_slice*>(d.records), d.prefix, table.n, table.total, target,
                                                      (decode_flags & 32u) != 0 /* cDecodeFlagsHighQuality */, channel0 < 0 ? 0u : (uint32_t)channel0,
                                                      channel1 < 0 ? 3u : (uint32_t)channel1, d_out, d.counters));
    }
    return out_invalid_per_slice ? read_back(ctx, out_invalid_per_slice, d.counters, (size_t)table.n * sizeof(uint32_t)) : 1;
}

// ---- the texture family: the two entries above with the further targets of uastc_transcode.h (ETC1, ETC2 RGBA, EAC R11 / RG11, the 16-bit rasters). The first
// family keeps its seven targets and its refusals; these run the same code behind their own target list, flag check and names.
static const char* const kUastcTextureTargets = "ETC1_RGB 0, ETC2_RGBA 1, BC1_RGB 2, BC3_RGBA 3, BC4_R 4, BC5_RG 5, BC7_RGBA 6, ASTC_4x4_RGBA 10, RGBA32 13, RGB565 14, BGR565 15, "
                                                "RGBA4444 16, ETC2_EAC_R11 20, ETC2_EAC_RG11 21";

// the refusals both texture entries share, before any pointer is looked at: the target, then every decode flag but cDecodeFlagsHighQuality, each by its name
static int uastc_texture_ok(bu_hip_context* ctx, const char* fn, uint32_t target, uint32_t decode_flags) {
    if (!bu::uastc_texture_unit_bytes(target)) {
        set_error(ctx, "%s: target %u (%s) is not supported (supported: %s)", fn, target, transcoder_format_name(target), kUastcTextureTargets);
        return 0;
    }
    const uint32_t refused = decode_flags & ~32u;
    if (refused) {
        static const struct { uint32_t bit; const char* name; } flags[] = {
            { 2, "cDecodeFlagsPVRTCDecodeToNextPow2" }, { 4, "cDecodeFlagsTranscodeAlphaDataToOpaqueFormats" }, { 8, "cDecodeFlagsBC1ForbidThreeColorBlocks" },
            { 16, "cDecodeFlagsOutputHasAlphaIndices" }, { 64, "cDecodeFlagsNoETC1SChromaFiltering" }, { 128, "cDecodeFlagsNoDeblockFiltering" },
            { 512, "cDecodeFlagsForceDeblockFiltering" }, { 1024, "cDecodeFlagXUASTCLDRDisableFastBC7Transcoding" } };
        char names[320] = "";
        uint32_t unnamed = refused;
        for (const auto& f : flags)
            if (refused & f.bit) {
                snprintf(names + strlen(names), sizeof(names) - strlen(names), "%s%s", names[0] ? ", " : "", f.name);
                unnamed &= ~f.bit;
            }
        if (unnamed) snprintf(names + strlen(names), sizeof(names) - strlen(names), "%sunnamed bits 0x%x", names[0] ? ", " : "", unnamed);
        set_error(ctx, "%s: decode_flags 0x%x: %s not supported (supported: 32, cDecodeFlagsHighQuality)", fn, decode_flags, names);
        return 0;
    }
    return 1;
}

size_t bu_hip_uastc_texture_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_width, uint32_t orig_height, uint32_t target, uint32_t out_row_pitch_pixels,
                                         uint32_t out_rows_pixels) {
    return bu::raster_output_bytes(bu::tile_geometry{ nbx, nby, orig_width, orig_height, out_row_pitch_pixels, out_rows_pixels }, bu::uastc_texture_unit_bytes(target),
                                   bu::uastc_texture_is_pixel_target(target));
}

int bu_hip_k_transcode_uastc_texture(bu_hip_context* ctx, const void* d_blocks, uint32_t nbx, uint32_t nby, uint32_t orig_width, uint32_t orig_height, uint32_t target,
                                     uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels,
                                     uint32_t* out_invalid_blocks) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_uastc_texture";
    if (out_invalid_blocks) *out_invalid_blocks = 0;
    if (!uastc_texture_ok(ctx, fn, target, decode_flags)) return 0;
    if (channel0 > 3 || channel1 > 3) { set_error(ctx, "%s: channel out of range", fn); return 0; }
    bu::tile_geometry geo;
    if (!checked(ctx, [&](bu::err_text e) {
            return bu::resolve_geometry(fn, nbx, nby, orig_width, orig_height, out_row_pitch_pixels, out_rows_pixels, bu::kUastcOneImage, &geo, e);
        })) return 0;
    if (!bu::uastc_texture_is_pixel_target(target) && (out_row_pitch_pixels || out_rows_pixels)) {
        set_error(ctx, "%s: row pitch %u / rows %u given for a block target (%s): they describe a pixel raster", fn, out_row_pitch_pixels, out_rows_pixels,
                  transcoder_format_name(target));
        return 0;
    }
    if (!nbx || !nby) return 1;   // no blocks: nothing is launched
    if (!d_blocks || !d_out) { set_error(ctx, "%s: null device pointer", fn); return 0; }
    const uint32_t unit = bu::uastc_texture_unit_bytes(target);
    if (((uintptr_t)d_blocks & 15u) || ((uintptr_t)d_out & (unit - 1))) {   // a block is loaded, and a block or pixel stored, as whole words
        set_error(ctx, "%s: the blocks must be 16-byte aligned and the output aligned to its %u-byte unit", fn, unit);
        return 0;
    }
    device_guard g(ctx->device);
    arena& counter = ctx->scratch[4];
    BU_TRY(ctx, counter.reserve(sizeof(uint32_t)));
    {
        prof_scope ps(ctx, "uastc_transcode_texture");
        BU_TRY(ctx, bu::launch_transcode_uastc(ctx->stream, d_blocks, geo, target, (decode_flags & 32u) != 0, channel0 < 0 ? 0u : (uint32_t)channel0,
                                               channel1 < 0 ? 3u : (uint32_t)channel1, d_out, static_cast<uint32_t*>(counter.p), true));
    }
    uint32_t invalid = 0;
    if (!read_back(ctx, &invalid, counter.p, sizeof(invalid))) return 0;
    if (out_invalid_blocks) *out_invalid_blocks = invalid;
    return 1;
}

int bu_hip_k_transcode_uastc_textures(bu_hip_context* ctx, const void* d_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
                                      uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice) {
    if (!ctx) return 0;
    static const char* const fn = "transcode_uastc_textures";
    if (!uastc_texture_ok(ctx, fn, target, decode_flags)) return 0;
    if (!d_blocks) { set_error(ctx, "%s: null pointer", fn); return 0; }
    if ((uintptr_t)d_blocks & 15u) { set_error(ctx, "%s: the blocks are not 16-byte aligned", fn); return 0; }
    if (channel0 > 3 || channel1 > 3) { set_error(ctx, "%s: channel out of range", fn); return 0; }
    bu::slice_table table;
    if (!uastc_texture_slices_check(ctx, table, fn, slices, n_slices, n_blocks, target, d_out, out_bytes)) return 0;
    device_guard g(ctx->device);
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    {
        prof_scope ps(ctx, fn);
        BU_TRY(ctx, bu::launch_transcode_uastc_slices(ctx->stream, d_blocks, static_cast<const bu_hip_transcode_slice*>(d.records), d.prefix, table.n, table.total, target,
                                                      (decode_flags & 32u) != 0, channel0 < 0 ? 0u : (uint32_t)channel0, channel1 < 0 ? 3u : (uint32_t)channel1, d_out,
                                                      d.counters, true));
    }
    return out_invalid_per_slice ? read_back(ctx, out_invalid_per_slice, d.counters, (size_t)table.n * sizeof(uint32_t)) : 1;
}

void bu_hip_uastc_rdo_default_params(bu_uastc_rdo_params* p) {
    if (!p) return;
    p->m_lz_dict_size = 4096; p->m_lambda = 0.5f; p->m_max_allowed_rms_increase_ratio = 10.0f; p->m_skip_block_rms_thresh = 8.0f;
    p->m_endpoint_refinement = 1; p->m_lz_literal_cost = 100; p->m_max_smooth_block_std_dev = 18.0f; p->m_smooth_block_max_error_scale = 10.0f;
}

// uastc_rdo's asserts (uastc_enc.cpp:4097-4099) as errors
static bool uastc_rdo_params_ok(bu_hip_context* ctx, const bu_uastc_rdo_params* params) {
    if (params->m_max_allowed_rms_increase_ratio > 1.0f && params->m_lz_dict_size && params->m_lambda > 0.0f) return true;
    set_error(ctx, "uastc_rdo: need max_allowed_rms_increase_ratio > 1, lz_dict_size > 0, lambda > 0");
    return false;
}

// The strip walks of uastc_rdo behind its prepare pass: the lean build (strips without a block of a sensitive mode: four waves per SIMD) on the context's stream and,
// when endpoint refinement is on, the build with the refit in it (the flagged strips) on the side stream beside it -- forked and joined with events, nobody waits on
// the host. Without a side stream the two launches simply follow each other.
// launch(stream, phase): one build of the walk (phase 1 lean, 3 with the refit) over the call's strips
extern "C++" template <class Launch>
static int uastc_rdo_walks(bu_hip_context* ctx, bool refit, Launch launch) {
    if (ctx->walk_stream) {
        // a pipeline lane with reserved walk CUs: both builds of the walk on streams of their own whose CU masks are the reserved set, forked off and joined back to the
        // lane's stream (which may not use those CUs): the walks' waves never wait for a slot behind a chip-filling kernel, and never share a SIMD with one
        BU_TRY(ctx, hipEventRecord(ctx->side_fork, ctx->stream));
        BU_TRY(ctx, hipStreamWaitEvent(ctx->walk_stream, ctx->side_fork, 0));
        BU_TRY(ctx, launch(ctx->walk_stream, 1));
        BU_TRY(ctx, hipEventRecord(ctx->walk_join, ctx->walk_stream));
        if (refit) {
            BU_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
            BU_TRY(ctx, launch(ctx->side_stream, 3));
            BU_TRY(ctx, hipEventRecord(ctx->side_join, ctx->side_stream));
            BU_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_join, 0));
        }
        BU_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->walk_join, 0));
        return 1;
    }
    const bool side = refit && ensure_side_stream(ctx);
    if (side) {
        BU_TRY(ctx, hipEventRecord(ctx->side_fork, ctx->stream));
        BU_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
        BU_TRY(ctx, launch(ctx->side_stream, 3));
        BU_TRY(ctx, hipEventRecord(ctx->side_join, ctx->side_stream));
    }
    BU_TRY(ctx, launch(ctx->stream, 1));
    if (side) BU_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_join, 0));
    else if (refit) BU_TRY(ctx, launch(ctx->stream, 3));
    return 1;
}

// bu_uastc_rdo_params as everything below the C ABI takes it
static bu_uastc::rdo_params uastc_rdo_kernel_params(const bu_uastc_rdo_params* q) {
    return { q->m_lambda, q->m_max_allowed_rms_increase_ratio, q->m_skip_block_rms_thresh, q->m_max_smooth_block_std_dev, q->m_smooth_block_max_error_scale,
             q->m_lz_dict_size, q->m_lz_literal_cost, q->m_endpoint_refinement };
}

// THE run of uastc_rdo over the strips of L, behind its entries' checks: prepare, both builds of the walk, finish, counters.
//   table: the strip table form, records and order uploaded first; otherwise the arithmetic form, for a layout of one slice
//   h_pinned_counters == nullptr: the call waits -- for the strip counts that size the finish and for the counters; a block that does not unpack fails it in the
//     text of the single-slice entry (named_slice < 0) or naming slice named_slice + its slice of L; out_stats (may be nullptr): {modified, refined, skipped} into
//     the first three words of every slice's row of four
//   h_pinned_counters != nullptr: nothing waits -- the finish is launched for the longest list a strip can have (every block of it modified: surplus workgroups
//     leave at once) and the four counters of slice 0 travel to the pinned words behind it. (The scopes record nothing there: a pipeline lane never profiles.)
static int uastc_rdo_run(bu_hip_context* ctx, void* d_blocks, const void* d_px, const bu::rdo_slices_layout& L, const bu_uastc::rdo_params& p, uint32_t flags, bool table,
                         uint32_t* h_pinned_counters, int64_t named_slice, uint32_t* out_stats) {
    static const char* const scopes[2][3] = { { "uastc_rdo_prepare", "uastc_rdo_strips", "uastc_rdo_finish" },
                                              { "uastc_rdo_slices_prepare", "uastc_rdo_slices_strips", "uastc_rdo_slices_finish" } };
    arena& ws = ctx->scratch[5];
    BU_TRY(ctx, ws.reserve(L.total_bytes));
    char* base = static_cast<char*>(ws.p);
    if (table) {
        BU_TRY(ctx, h2d(ctx, base + L.strips, L.recs.data(), L.recs.size() * sizeof(bu::rdo_strip_rec)));
        BU_TRY(ctx, h2d(ctx, base + L.order_at, L.order.data(), L.order.size() * 4));
    }
    {
        prof_scope ps(ctx, scopes[table][0]);
        BU_TRY(ctx, bu::launch_uastc_rdo_prepare(ctx->stream, d_blocks, d_px, L, p, ws.p, table));
    }
    {
        prof_scope ps(ctx, scopes[table][1]);   // both walks: the scope ends behind the join
        if (!uastc_rdo_walks(ctx, p.endpoint_refinement != 0, [&](hipStream_t st, int build) { return bu::launch_uastc_rdo_walk(st, build == 3, d_blocks, d_px, L, p, ws.p, table); }))
            return 0;
    }
    uint32_t longest = L.longest;
    if (!h_pinned_counters) {
        // how many blocks each strip modified: sizes the finish launch (one download for all slices; the walks have to be over anyway)
        std::vector<uint32_t> per_strip(L.recs.size());
        if (!fetch(ctx, per_strip.data(), base + L.strip_counts, per_strip.size() * 4)) return 0;
        longest = *std::max_element(per_strip.begin(), per_strip.end());
    }
    {
        prof_scope ps(ctx, scopes[table][2]);
        BU_TRY(ctx, bu::launch_uastc_rdo_finish(ctx->stream, d_blocks, d_px, L, p, flags, ws.p, table, longest));
    }
    if (h_pinned_counters) {
        BU_TRY(ctx, hipMemcpyAsync(h_pinned_counters, base + L.counters, 16, hipMemcpyDeviceToHost, ctx->stream));
        return 1;
    }
    std::vector<uint32_t> counters((size_t)L.n_slices * 4);   // per slice: modified, failed, refined, skipped
    if (!fetch(ctx, counters.data(), base + L.counters, counters.size() * 4)) return 0;
#ifdef RDO_PROFILE
    if (!table) {
        unsigned long long prof[16];
        (void)hipMemcpy(prof, base + L.counters + 64, sizeof(prof), hipMemcpyDeviceToHost);
        fprintf(stderr, "rdo strip 0 cycles by phase:");
        for (int k = 0; k < 16; k++) fprintf(stderr, " %llu", prof[k]);
        fprintf(stderr, "\n");
    }
#endif
    for (uint32_t s = 0; s < L.n_slices; s++)
        if (counters[4 * s + 1]) {
            if (named_slice < 0) set_error(ctx, "uastc_rdo: a block does not unpack as UASTC");
            else set_error(ctx, "uastc_rdo_slices: a block of slice %u does not unpack as UASTC", (uint32_t)(named_slice + s));
            return 0;
        }
    if (out_stats)
        for (uint32_t s = 0; s < L.n_slices; s++) { out_stats[4 * s] = counters[4 * s]; out_stats[4 * s + 1] = counters[4 * s + 2]; out_stats[4 * s + 2] = counters[4 * s + 3]; }
    return 1;
}

int bu_hip_k_uastc_rdo(bu_hip_context* ctx, void* d_blocks, const void* d_px, uint32_t n_blocks, const bu_uastc_rdo_params* params, uint32_t flags,
                       uint32_t total_jobs, uint32_t out_stats[4]) {
    if (!ctx) return 0;
    if (!d_blocks || !d_px || !params) { set_error(ctx, "uastc_rdo: null pointer"); return 0; }
    if (!uastc_rdo_params_ok(ctx, params)) return 0;
    bu::rdo_slices_layout L;
    if (!bu::rdo_slice_layout_build(n_blocks, total_jobs, L)) { set_error(ctx, "uastc_rdo: more than %u blocks", bu::RDO_SLICES_MAX_BLOCKS); return 0; }
    device_guard g(ctx->device);
    if (out_stats) out_stats[0] = out_stats[1] = out_stats[2] = 0, out_stats[3] = L.slice_strips[0];
    if (!n_blocks) return 1;
    return uastc_rdo_run(ctx, d_blocks, d_px, L, uastc_rdo_kernel_params(params), flags, false, nullptr, -1, out_stats);
}

size_t bu_hip_uastc_rdo_slices_workspace_bytes(const uint32_t* slice_blocks, uint32_t n_slices, uint32_t total_jobs) {
    bu::rdo_slices_layout L;
    if (!slice_blocks || !n_slices || !bu::rdo_slices_layout_build(slice_blocks, n_slices, total_jobs, L)) return 0;
    return L.total_bytes;
}

// bu_hip_k_uastc_rdo over every slice of a file in one pass: the strips of all slices walk side by side (one prepare launch, one launch per build of the walk,
// one finish launch), and the host waits twice whatever n_slices is: for the strip counts that size the finish, and for the counters.
int bu_hip_k_uastc_rdo_slices(bu_hip_context* ctx, void* d_blocks, const void* d_px, const uint32_t* slice_blocks, uint32_t n_slices, const bu_uastc_rdo_params* params,
                              uint32_t flags, uint32_t total_jobs, uint32_t* out_stats) {
    if (!ctx) return 0;
    if (!d_blocks || !d_px || !slice_blocks || !params) { set_error(ctx, "uastc_rdo_slices: null pointer"); return 0; }
    if (!n_slices) { set_error(ctx, "uastc_rdo_slices: no slices"); return 0; }
    bu::rdo_slices_layout L;
    if (!bu::rdo_slices_layout_build(slice_blocks, n_slices, total_jobs, L)) { set_error(ctx, "uastc_rdo_slices: more than %u blocks in all", bu::RDO_SLICES_MAX_BLOCKS); return 0; }
    if (!uastc_rdo_params_ok(ctx, params)) return 0;
    device_guard g(ctx->device);
    if (out_stats)
        for (uint32_t s = 0; s < n_slices; s++) out_stats[4 * s] = out_stats[4 * s + 1] = out_stats[4 * s + 2] = 0, out_stats[4 * s + 3] = L.slice_strips[s];
    if (!L.total_blocks) return 1;
    const bu_uastc::rdo_params p = uastc_rdo_kernel_params(params);
    const uint32_t s = L.recs.front().slice;
    if (L.recs.back().slice != s) return uastc_rdo_run(ctx, d_blocks, d_px, L, p, flags, true, nullptr, 0, out_stats);
    // ONE slice holds all the blocks (a bare image without mips; the slices in front of it are empty, so it begins where the call's arrays do): nothing to overlap,
    // and the arithmetic builds of the walk were measured 0.4 - 0.9 % faster per block than the strip table's on a 4096^2 chain -- the call runs on the
    // layout of that slice alone, launch for launch what bu_hip_k_uastc_rdo does with it
    bu::rdo_slices_layout one;
    bu::rdo_slice_layout_build(slice_blocks[s], total_jobs, one);   // fits: L does
    return uastc_rdo_run(ctx, d_blocks, d_px, one, p, flags, false, nullptr, s, out_stats ? out_stats + 4 * (size_t)s : nullptr);
}

bu_uastc_pipeline* bu_hip_uastc_pipeline_create(bu_hip_context* ctx, uint32_t lanes, uint32_t max_blocks, uint32_t flags, uint32_t max_total_jobs) {
    if (!ctx) return nullptr;
    if (lanes < 1 || lanes > 8 || !max_blocks) { set_error(ctx, "uastc_pipeline_create: 1..8 lanes, max_blocks > 0"); return nullptr; }
    device_guard g(ctx->device);
    bu_uastc_pipeline* p = new (std::nothrow) bu_uastc_pipeline();
    if (!p) return nullptr;
    p->parent = ctx;
    p->lanes.resize(lanes);
    // every workspace at its final size now: growing one later would free it under the kernels of an earlier submission
    const size_t ws_bytes = p->ws_bytes = std::max(bu::uastc_workspace_bytes(max_blocks, flags), bu::uastc_rdo_workspace_bytes(max_blocks, max_total_jobs));
    for (auto& l : p->lanes) {
        l.ctx = create_context_kind(ctx->device, true);
        if (l.ctx) {
            l.ctx->tuning = ctx->tuning;   // the lanes take the paths their parent context is set to
            // The runtime maps ordinary streams onto its few shared hardware queues (GPU_MAX_HW_QUEUES) by how many streams each queue already carries -- history, as far
            // as a library can tell -- and two lanes whose streams share a queue run one after the other. A stream with a CU mask gets a hardware queue of its OWN: the
            // lanes' streams are made with one that enables every CU.
            const uint32_t walk_cus = ctx->tuning.uastc_walk_cus;
            if (!l.ctx->dedicated_queue || l.ctx->walk_cus != walk_cus) {
                hipStream_t fresh = make_dedicated_stream(l.ctx->device, walk_cus, false);
                if (fresh) {
                    (void)hipStreamSynchronize(l.ctx->own_stream);
                    const bool own = l.ctx->stream == l.ctx->own_stream;
                    (void)hipStreamDestroy(l.ctx->own_stream);
                    l.ctx->own_stream = fresh; l.ctx->dedicated_queue = true;
                    if (own) l.ctx->stream = fresh;
                    // the walks' streams: on the reserved CUs (or gone, when nothing is reserved)
                    if (l.ctx->walk_stream) { (void)hipStreamSynchronize(l.ctx->walk_stream); (void)hipStreamDestroy(l.ctx->walk_stream); l.ctx->walk_stream = nullptr; }
                    if (l.ctx->side_stream) { (void)hipStreamSynchronize(l.ctx->side_stream); (void)hipStreamDestroy(l.ctx->side_stream); l.ctx->side_stream = nullptr; }
                    l.ctx->walk_cus = 0;
                    if (walk_cus) {
                        l.ctx->walk_stream = make_dedicated_stream(l.ctx->device, walk_cus, true);
                        l.ctx->side_stream = make_dedicated_stream(l.ctx->device, walk_cus, true);
                        bool ok = l.ctx->walk_stream && l.ctx->side_stream;
                        if (ok && !l.ctx->walk_join) ok = hipEventCreateWithFlags(&l.ctx->walk_join, hipEventDisableTiming) == hipSuccess;
                        if (ok && !l.ctx->side_fork) ok = hipEventCreateWithFlags(&l.ctx->side_fork, hipEventDisableTiming) == hipSuccess;
                        if (ok && !l.ctx->side_join) ok = hipEventCreateWithFlags(&l.ctx->side_join, hipEventDisableTiming) == hipSuccess;
                        if (ok) l.ctx->walk_cus = walk_cus;
                        else {   // fall back to the unreserved form rather than fail: the lane's own stream keeps its (restricted) mask, the walks share it
                            (void)hipGetLastError();
                            if (l.ctx->walk_stream) { (void)hipStreamDestroy(l.ctx->walk_stream); l.ctx->walk_stream = nullptr; }
                            if (l.ctx->side_stream) { (void)hipStreamDestroy(l.ctx->side_stream); l.ctx->side_stream = nullptr; }
                        }
                    }
                }
            }
        }
        if (!l.ctx || hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&l.input, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&l.stats), 64, hipHostMallocDefault) != hipSuccess || l.ctx->scratch[5].reserve(ws_bytes) != hipSuccess) {
            set_error(ctx, "uastc_pipeline_create: lane set-up failed (%s)", l.ctx ? bu_hip_last_error(l.ctx) : "no context");
            bu_hip_uastc_pipeline_destroy(p);
            return nullptr;
        }
    }
    return p;
}

static int uastc_pipeline_collect(bu_uastc_pipeline* p, bu_uastc_pipeline::lane& l, uint32_t out_stats[4]) {
    if (!l.busy) return 1;
    if (hipEventSynchronize(l.done) != hipSuccess) { set_error(p->parent, "uastc_pipeline: a submission failed on the device"); l.busy = false; return 0; }
    l.busy = false;
    if (out_stats) { out_stats[0] = l.with_rdo ? l.stats[0] : 0; out_stats[1] = l.with_rdo ? l.stats[2] : 0; out_stats[2] = l.with_rdo ? l.stats[3] : 0; out_stats[3] = l.strips; }
    if (l.with_rdo && l.stats[1]) { set_error(p->parent, "uastc_rdo: a block does not unpack as UASTC"); return 0; }
    return 1;
}

int bu_hip_uastc_pipeline_submit(bu_uastc_pipeline* p, const void* d_px, uint32_t n_blocks, void* d_out, const bu_uastc_rdo_params* rdo, uint32_t flags, uint32_t total_jobs,
                                 uint64_t* out_ticket) {
    if (!p) return 0;
    bu_hip_context* ctx = p->parent;
    if (!d_px || !d_out || !n_blocks) { set_error(ctx, "uastc_pipeline_submit: null pointer / no blocks"); return 0; }
    // every refusal comes before the first enqueue: a submission that fails here has left nothing in flight on its lane, which wait() would not know to wait for
    bu::rdo_slices_layout L;
    if (rdo && !bu::rdo_slice_layout_build(n_blocks, total_jobs, L)) { set_error(ctx, "uastc_pipeline_submit: more than %u blocks", bu::RDO_SLICES_MAX_BLOCKS); return 0; }
    const size_t need = std::max(bu::uastc_workspace_bytes(n_blocks, flags), L.total_bytes);
    if (need > p->ws_bytes) { set_error(ctx, "uastc_pipeline_submit: %u blocks / %u jobs exceed what the pipeline was created for", n_blocks, total_jobs); return 0; }
    if (rdo && !uastc_rdo_params_ok(ctx, rdo)) return 0;
    device_guard g(ctx->device);
    const uint64_t ticket = p->next_ticket;
    bu_uastc_pipeline::lane& l = p->lanes[(size_t)(ticket % p->lanes.size())];
    if (!uastc_pipeline_collect(p, l, nullptr)) return 0;   // the lane's previous submission (its results are complete from here on; nobody asked for its statistics)
    // the input tiles may still be being produced on the caller's stream
    BU_TRY(ctx, hipEventRecord(l.input, ctx->stream));
    BU_TRY(ctx, hipStreamWaitEvent(l.ctx->stream, l.input, 0));
    if (!bu_hip_k_encode_uastc_blocks(l.ctx, d_px, n_blocks, flags, d_out)) { set_error(ctx, "uastc_pipeline_submit: %s", bu_hip_last_error(l.ctx)); return 0; }
    l.with_rdo = rdo != nullptr;
    l.strips = rdo ? L.slice_strips[0] : 0;
    if (rdo && !uastc_rdo_run(l.ctx, d_out, d_px, L, uastc_rdo_kernel_params(rdo), flags, false, l.stats, -1, nullptr)) { set_error(ctx, "uastc_pipeline_submit: %s", bu_hip_last_error(l.ctx)); return 0; }
    BU_TRY(ctx, hipEventRecord(l.done, l.ctx->stream));
    l.busy = true; l.ticket = ticket;
    p->next_ticket++;
    if (out_ticket) *out_ticket = ticket;
    return 1;
}

int bu_hip_uastc_pipeline_wait(bu_uastc_pipeline* p, uint64_t ticket, uint32_t out_stats[4]) {
    if (!p) return 0;
    if (out_stats) out_stats[0] = out_stats[1] = out_stats[2] = out_stats[3] = 0;
    device_guard g(p->parent->device);
    int ok = 1;
    for (auto& l : p->lanes)
        if (l.busy && (ticket == 0 || l.ticket == ticket)) ok &= uastc_pipeline_collect(p, l, ticket ? out_stats : nullptr);
    return ok;
}

void bu_hip_uastc_pipeline_destroy(bu_uastc_pipeline* p) {
    if (!p) return;
    for (auto& l : p->lanes) {
        if (l.ctx) { device_guard g(l.ctx->device); (void)hipStreamSynchronize(l.ctx->stream); }
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.input) (void)hipEventDestroy(l.input);
        if (l.stats) (void)hipHostFree(l.stats);
        if (l.ctx) bu_hip_destroy_context(l.ctx);
    }
    delete p;
}

int bu_hip_uastc_rdo(bu_hip_context* ctx, bu_uastc_block* blocks, const bu_uastc_rdo_params* params, uint32_t flags, uint32_t total_jobs, uint32_t out_stats[4]) {
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    if (!blocks) { set_error(ctx, "uastc_rdo: null blocks"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    arena& o = ctx->scratch[0];
    BU_TRY(ctx, o.reserve((size_t)n * 16));
    BU_TRY(ctx, h2d(ctx, o.p, blocks, (size_t)n * 16));
    if (!bu_hip_k_uastc_rdo(ctx, o.p, ctx->d_pixel_blocks, n, params, flags, total_jobs, out_stats)) return 0;
    if (!fetch(ctx, blocks, o.p, (size_t)n * 16)) return 0;
    return 1;
}
} // extern "C"
