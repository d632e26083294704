// api_image_metrics.cpp -- image_metrics::calc's counts behind the C ABI of libbasisu_hip.so: two resident RGBA8 rasters -> histograms + channel sums on the host.
#include "api_internal.h"
#include "image_metrics_kernels.h"
#include <cstddef>

static_assert(sizeof(bu_image_metrics_counts) - offsetof(bu_image_metrics_counts, hist) == sizeof(bu::image_metrics_device_counts), "the device counts are the struct's tail");

extern "C" {

int bu_hip_k_image_metrics(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                           bu_image_metrics_counts* h_out) {
    if (!ctx) return 0;
    if (!d_a || !d_b || !h_out) { set_error(ctx, "image_metrics: null pointer"); return 0; }
    if (h_out->struct_bytes < sizeof(uint32_t)) { set_error(ctx, "image_metrics: struct_bytes is not set"); return 0; }
    uint32_t pa = pitch_a, pb = pitch_b, w, h;
    if (!checked(ctx, [&](bu::err_text e) { return bu::raster_pair_region("image_metrics", d_a, wa, ha, &pa, d_b, wb, hb, &pb, &w, &h, bu::kImageMetricsMaxDim, e); })) return 0;
    device_guard g(ctx->device);
    arena& dev = ctx->scratch[4];
    BU_TRY(ctx, dev.reserve(sizeof(bu::image_metrics_device_counts)));
    {
        prof_scope ps(ctx, "image_metrics");
        BU_TRY(ctx, bu::launch_image_metrics(ctx->stream, static_cast<const uint32_t*>(d_a), pa, static_cast<const uint32_t*>(d_b), pb, w, h,
                                             static_cast<bu::image_metrics_device_counts*>(dev.p)));
    }
    bu_image_metrics_counts full;
    if (!read_back(ctx, full.hist, dev.p, sizeof(bu::image_metrics_device_counts))) return 0;
    full.struct_bytes = h_out->struct_bytes;
    full.width = w; full.height = h; full.reserved = 0;
    memcpy(h_out, &full, std::min<size_t>(h_out->struct_bytes, sizeof(full)));
    return 1;
}

} // extern "C"
