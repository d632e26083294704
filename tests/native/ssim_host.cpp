// ssim_host.cpp -- TEST-ONLY host build of csrc/ssim.h: the per-pixel arithmetic under a serial loop over two rasters, the plain serial mean, and the reduction's
// chunked walk (fsum_scan.h) next to the serial sum it must reproduce. Built and bound by tests/native_libs.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../basis_universal_amd/csrc/ssim_reduce.h"
#include "host_api.h"

namespace {

struct raster_at {
    const uint8_t *a, *b;
    uint32_t pitch_a, pitch_b, w, h, x, y;
    bool luma;
    void operator()(int xd, int yd, uint32_t& sa, uint32_t& sb) const {
        const int64_t cx = (int64_t)x + xd, cy = (int64_t)y + yd;
        const uint32_t px = cx < 0 ? 0 : (cx >= (int64_t)w ? w - 1 : (uint32_t)cx), py = cy < 0 ? 0 : (cy >= (int64_t)h ? h - 1 : (uint32_t)cy);
        uint32_t pa, pb;
        memcpy(&pa, a + ((size_t)py * pitch_a + px) * 4, 4);
        memcpy(&pb, b + ((size_t)py * pitch_b + px) * 4, 4);
        sa = luma ? bu::ssim_sample<2>(pa) : bu::ssim_sample<4>(pa);
        sb = luma ? bu::ssim_sample<2>(pb) : bu::ssim_sample<4>(pb);
    }
};

}  // namespace

HOST_API void ssh_weights(float* out121) { bu::ssim_gaussian_weights(out121); }

// a, b: RGBA8 rasters, pitches in pixels; the region is min(wa, wb) x min(ha, hb) and coordinates are clamped to IT. mode 0: out[pixel * 4 + channel], the RGBA call;
// mode 1 / 2: out[pixel], channel 0 of the 709 / 601 luma call. Pixels in raster order. Returns the number of pixels.
HOST_API uint64_t ssh_map(const uint8_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint8_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b, uint32_t mode, float* out) {
    const uint32_t w = wa < wb ? wa : wb, h = ha < hb ? ha : hb;
    if (!w || !h || mode >= bu::SSIM_MODES) return 0;
    bu::ssim_weights k;
    bu::ssim_gaussian_weights(k.w);
    raster_at at{a, b, pitch_a, pitch_b, w, h, 0, 0, mode != 0};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            at.x = x; at.y = y;
            const size_t i = (size_t)y * w + x;
            if (mode == 0) bu::ssim_pixel<4>(at, k, out + i * 4);
            else {
                float both[2];
                bu::ssim_pixel<2>(at, k, both);
                out[i] = both[mode - 1];
            }
        }
    return (uint64_t)w * h;
}

// the seven figures in the tool's order: R, G, B, RGB Avg, A, Y 709, Y 601. Returns 0 for an empty region.
HOST_API int ssh_ssim(const uint8_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint8_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b, float* out7) {
    const uint32_t w = wa < wb ? wa : wb, h = ha < hb ? ha : hb;
    if (!w || !h) return 0;
    const size_t n = (size_t)w * h;
    std::vector<float> rgba(n * 4), plane(n);
    float s[4];
    ssh_map(a, wa, ha, pitch_a, b, wb, hb, pitch_b, 0, rgba.data());
    for (int c = 0; c < 4; c++) {
        for (size_t i = 0; i < n; i++) plane[i] = rgba[i * 4 + c];
        s[c] = bu::ssim_avg(plane.data(), n);
    }
    out7[0] = s[0]; out7[1] = s[1]; out7[2] = s[2];
    out7[3] = (s[0] + s[1] + s[2]) / 3.0f;
    out7[4] = s[3];
    for (uint32_t mode = 1; mode < 3; mode++) {
        ssh_map(a, wa, ha, pitch_a, b, wb, hb, pitch_b, mode, plane.data());
        out7[4 + mode] = bu::ssim_avg(plane.data(), n);
    }
    return 1;
}

// the serial running sum from 0, not divided
HOST_API float ssh_serial_sum(const float* v, uint64_t n) {
    volatile float s = 0.0f;
    for (uint64_t i = 0; i < n; i++) s = s + v[i];
    return s;
}

// The reduction as the device runs it: per chunk a double sum, an exclusive prefix of those, a chunk summary from the prefix (scaled by prefix_scale: 1 is the device's
// guess, anything else a deliberately bad one), then the ordered walk. stats[0] = chunks, stats[1] = chunks whose addends were added one by one.
HOST_API float ssh_chunked_sum(const float* v, uint64_t n, uint32_t chunk, double prefix_scale, uint64_t* stats) {
    const uint64_t chunks = (n + chunk - 1) / chunk;
    std::vector<bu::ssim_chunk> sm(chunks);
    double prefix = 0.0;
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t i0 = c * chunk;
        const uint32_t len = (uint32_t)(n - i0 < chunk ? n - i0 : chunk);
        sm[c] = bu::ssim_chunk_build(v + i0, len, prefix * prefix_scale);
        double t = 0.0;
        for (uint32_t i = 0; i < len; i++) t += (double)v[i0 + i];
        prefix += t;
    }
    uint32_t state = 0, walked = 0;
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t i0 = c * chunk;
        state = bu::ssim_chunk_walk(state, sm[c], v + i0, (uint32_t)(n - i0 < chunk ? n - i0 : chunk), &walked);
    }
    if (stats) { stats[0] = chunks; stats[1] = walked; }
    return bu::ssim_float(state);
}
