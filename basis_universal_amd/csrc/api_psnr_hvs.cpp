// api_psnr_hvs.cpp -- psnr_hvs_compute_metrics' block sums behind the C ABI of libbasisu_hip.so: two resident RGBA8 rasters -> twelve doubles on the host, and the
// per-block doubles of one mode for tests.
#include "api_internal.h"
#include "image_metrics_kernels.h"
#include "psnr_hvs_kernels.h"
#include <cstddef>

static_assert(sizeof(bu_psnr_hvs_sums) - offsetof(bu_psnr_hvs_sums, sum_hvs) == sizeof(bu::psnr_hvs_device_sums), "the device sums are the struct's tail");

// the checks both entry points share -> the region, or 0 with the error set
static int psnr_hvs_region(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t& pa, const void* d_b, uint32_t wb, uint32_t hb, uint32_t& pb, uint32_t& w,
                           uint32_t& h) {
    return checked(ctx, [&](bu::err_text e) { return bu::raster_pair_region("psnr_hvs", d_a, wa, ha, &pa, d_b, wb, hb, &pb, &w, &h, bu::kImageMetricsMaxDim, e); });
}

// launches into scratch[4] (sums, then partials) and, with per_block, scratch[5]; the sums are on the host and the stream idle when it returns 1
static int psnr_hvs_run(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pa, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pb, uint32_t blocks,
                        bool per_block, uint32_t mode, bu_psnr_hvs_sums& full) {
    device_guard g(ctx->device);
    arena& dev = ctx->scratch[4];
    const size_t head = 256;   // the sums, padded so that the partials stay aligned
    static_assert(sizeof(bu::psnr_hvs_device_sums) <= 256, "head");
    BU_TRY(ctx, dev.reserve(head + bu::psnr_hvs_partial_bytes()));
    if (per_block) BU_TRY(ctx, ctx->scratch[5].reserve((size_t)std::max(blocks, 1u) * 2 * sizeof(double)));
    {
        prof_scope ps(ctx, "psnr_hvs");
        BU_TRY(ctx, bu::launch_psnr_hvs(ctx->stream, static_cast<const uint32_t*>(d_a), wa, ha, pa, static_cast<const uint32_t*>(d_b), wb, hb, pb,
                                        reinterpret_cast<double*>(static_cast<char*>(dev.p) + head), static_cast<bu::psnr_hvs_device_sums*>(dev.p),
                                        per_block ? static_cast<double*>(ctx->scratch[5].p) : nullptr, mode));
    }
    return read_back(ctx, full.sum_hvs, dev.p, sizeof(bu::psnr_hvs_device_sums));
}

extern "C" {

int bu_hip_k_psnr_hvs(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                      bu_psnr_hvs_sums* h_out) {
    if (!ctx) return 0;
    if (!d_a || !d_b || !h_out) { set_error(ctx, "psnr_hvs: null pointer"); return 0; }
    if (h_out->struct_bytes < sizeof(uint32_t)) { set_error(ctx, "psnr_hvs: struct_bytes is not set"); return 0; }
    uint32_t w, h;
    if (!psnr_hvs_region(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, w, h)) return 0;
    bu_psnr_hvs_sums full;
    full.struct_bytes = h_out->struct_bytes;
    full.width = w; full.height = h; full.blocks = (w && h) ? bu::psnr_hvs_blocks(w, h) : 0;
    if (!psnr_hvs_run(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, full.blocks, false, 0, full)) return 0;
    memcpy(h_out, &full, std::min<size_t>(h_out->struct_bytes, sizeof(full)));
    return 1;
}

int bu_hip_k_psnr_hvs_blocks(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                             uint32_t mode, double* h_out_blocks, uint32_t capacity_blocks, uint32_t* out_blocks) {
    if (!ctx) return 0;
    if (!d_a || !d_b || !h_out_blocks) { set_error(ctx, "psnr_hvs_blocks: null pointer"); return 0; }
    if (mode >= 6) { set_error(ctx, "psnr_hvs_blocks: mode %u (0-5)", mode); return 0; }
    uint32_t w, h;
    if (!psnr_hvs_region(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, w, h)) return 0;
    const uint32_t blocks = (w && h) ? bu::psnr_hvs_blocks(w, h) : 0;
    if (blocks > capacity_blocks) { set_error(ctx, "psnr_hvs_blocks: %u blocks, room for %u", blocks, capacity_blocks); return 0; }
    bu_psnr_hvs_sums full;
    if (!psnr_hvs_run(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, blocks, true, mode, full)) return 0;
    if (blocks && !read_back(ctx, h_out_blocks, ctx->scratch[5].p, (size_t)blocks * 2 * sizeof(double))) return 0;
    if (out_blocks) *out_blocks = blocks;
    return 1;
}

} // extern "C"
