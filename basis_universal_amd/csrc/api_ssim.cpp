// api_ssim.cpp -- compute_ssim's seven figures behind the C ABI of libbasisu_hip.so: two resident RGBA8 rasters -> seven floats on the host, and the smap values of one
// call for tests. The six smap planes and the reduction's chunk tables live in scratch[5] for the length of the call.
#include "api_internal.h"
#include "image_metrics_kernels.h"
#include "ssim_kernels.h"
#include <cstddef>

// an arena this large is given back when the call ends: six planes of a 4096 x 4096 pair are 384 MiB, too much to keep for the context's life
static constexpr size_t kSsimKeepBytes = (size_t)64 << 20;

// the checks both entry points share -> the region, or 0 with the error set
static int ssim_region(bu_hip_context* ctx, const char* who, const void* d_a, uint32_t wa, uint32_t ha, uint32_t& pa, const void* d_b, uint32_t wb, uint32_t hb, uint32_t& pb,
                       uint32_t& w, uint32_t& h) {
    // the size limit is this file's own sentence (it names the pixel cap too), after the empty region's: none is given to the shared check
    if (!checked(ctx, [&](bu::err_text e) { return bu::raster_pair_region(who, d_a, wa, ha, &pa, d_b, wb, hb, &pb, &w, &h, UINT32_MAX, e); })) return 0;
    if (!w || !h) { set_error(ctx, "%s: an empty region (%u x %u pixels): there is no mean over no pixels", who, w, h); return 0; }
    if (w > bu::kImageMetricsMaxDim || h > bu::kImageMetricsMaxDim || (uint64_t)w * h > bu::kSsimMaxPixels) {
        set_error(ctx, "%s: a region of %u x %u pixels is too large (%u each way and %u pixels at the most: the context holds six float planes of the region)", who, w, h,
                  (uint32_t)bu::kImageMetricsMaxDim, (uint32_t)bu::kSsimMaxPixels);
        return 0;
    }
    return 1;
}

// the launches into scratch[5]; nothing has been waited for when it returns 1
static int ssim_run(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pa, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pb, uint32_t pixels, bool reduce) {
    static const bu::ssim_weights weights = [] { bu::ssim_weights k; bu::ssim_gaussian_weights(k.w); return k; }();   // host libm, once
    BU_TRY(ctx, ctx->scratch[5].reserve(bu::ssim_work_bytes(pixels)));
    prof_scope ps(ctx, "ssim");
    BU_TRY(ctx, bu::launch_ssim(ctx->stream, static_cast<const uint32_t*>(d_a), wa, ha, pa, static_cast<const uint32_t*>(d_b), wb, hb, pb, weights, ctx->scratch[5].p, reduce));
    return 1;
}

static void ssim_done(bu_hip_context* ctx) {
    if (ctx->scratch[5].cap > kSsimKeepBytes) ctx->scratch[5].release();   // the stream is idle: every caller has waited for its results
}

extern "C" {

int bu_hip_k_ssim(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                  bu_ssim_result* h_out) {
    if (!ctx) return 0;
    if (!d_a || !d_b || !h_out) { set_error(ctx, "ssim: null pointer"); return 0; }
    if (h_out->struct_bytes < sizeof(uint32_t)) { set_error(ctx, "ssim: struct_bytes is not set"); return 0; }
    uint32_t w, h;
    if (!ssim_region(ctx, "ssim", d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, w, h)) return 0;
    device_guard g(ctx->device);
    const uint32_t n = w * h;
    bu::ssim_device_result dev;
    int ok = ssim_run(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, n, true);
    if (ok) ok = read_back(ctx, &dev, static_cast<char*>(ctx->scratch[5].p) + bu::ssim_result_offset(n), sizeof(dev));
    ssim_done(ctx);
    if (!ok) return 0;
    bu_ssim_result full;
    full.struct_bytes = h_out->struct_bytes;
    full.width = w; full.height = h;
    full.chunks = bu::ssim_chunks(n) * bu::SSIM_PLANES;
    full.chunks_walked = 0;
    for (uint32_t p = 0; p < bu::SSIM_PLANES; p++) full.chunks_walked += dev.walked[p];
    full.r = dev.mean[bu::SSIM_PLANE_R]; full.g = dev.mean[bu::SSIM_PLANE_G]; full.b = dev.mean[bu::SSIM_PLANE_B];
    full.rgb = (full.r + full.g + full.b) / 3.0f;   // as the tool prints "RGB Avg SSIM"
    full.a = dev.mean[bu::SSIM_PLANE_A];
    full.luma_709 = dev.mean[bu::SSIM_PLANE_709]; full.luma_601 = dev.mean[bu::SSIM_PLANE_601];
    memcpy(h_out, &full, std::min<size_t>(h_out->struct_bytes, sizeof(full)));
    return 1;
}

int bu_hip_k_ssim_map(bu_hip_context* ctx, const void* d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const void* d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                      uint32_t mode, float* h_out, uint64_t capacity_floats, uint32_t* out_pixels) {
    if (!ctx) return 0;
    if (!d_a || !d_b || !h_out) { set_error(ctx, "ssim_map: null pointer"); return 0; }
    if (mode >= bu::SSIM_MODES) { set_error(ctx, "ssim_map: mode %u (0-2)", mode); return 0; }
    uint32_t w, h;
    if (!ssim_region(ctx, "ssim_map", d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, w, h)) return 0;
    const uint32_t n = w * h, per_pixel = mode == bu::SSIM_RGBA ? 4u : 1u;
    if ((uint64_t)n * per_pixel > capacity_floats) { set_error(ctx, "ssim_map: %llu floats, room for %llu", (unsigned long long)n * per_pixel, (unsigned long long)capacity_floats); return 0; }
    device_guard g(ctx->device);
    int ok = ssim_run(ctx, d_a, wa, ha, pitch_a, d_b, wb, hb, pitch_b, n, false);
    if (ok) {
        const float* planes = static_cast<const float*>(ctx->scratch[5].p);
        if (mode == bu::SSIM_RGBA) {
            std::vector<float> planar((size_t)n * 4);
            ok = read_back(ctx, planar.data(), planes, planar.size() * sizeof(float));
            if (ok)
                for (size_t i = 0; i < n; i++)
                    for (uint32_t c = 0; c < 4; c++) h_out[i * 4 + c] = planar[(size_t)c * n + i];
        } else {
            ok = read_back(ctx, h_out, planes + (size_t)(mode == bu::SSIM_LUMA_709 ? bu::SSIM_PLANE_709 : bu::SSIM_PLANE_601) * n, (size_t)n * sizeof(float));
        }
    }
    ssim_done(ctx);
    if (!ok) return 0;
    if (out_pixels) *out_pixels = n;
    return 1;
}

} // extern "C"
