// image_metrics_host.cpp -- TEST-ONLY host build of csrc/image_metrics.h: the per-pixel arithmetic the kernel counts with and the histogram -> metrics reduction the
// host library exports, under a serial loop over two rasters. Built and bound by tests/native_libs.py.
#include <cstdint>
#include <cstring>

#include "../../basis_universal_amd/csrc/image_metrics.h"
#include "host_api.h"

// a, b: RGBA8 rasters, pitches in pixels; the region is min(wa, wb) x min(ha, hb). hist[6 * 256], sum_a[4], sum_b[4] are overwritten.
HOST_API void imh_counts(const uint8_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint8_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b, uint32_t* hist, uint64_t* sum_a,
                uint64_t* sum_b) {
    memset(hist, 0, bu::IM_ROWS * bu::IM_BINS * sizeof(uint32_t));
    memset(sum_a, 0, 4 * sizeof(uint64_t));
    memset(sum_b, 0, 4 * sizeof(uint64_t));
    const uint32_t w = wa < wb ? wa : wb, h = ha < hb ? ha : hb;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            uint32_t pa, pb, bins[bu::IM_ROWS];
            memcpy(&pa, a + ((size_t)y * pitch_a + x) * 4, 4);
            memcpy(&pb, b + ((size_t)y * pitch_b + x) * 4, 4);
            bu::im_pixel_bins(pa, pb, bins);
            for (uint32_t r = 0; r < bu::IM_ROWS; r++) hist[r * bu::IM_BINS + bins[r]]++;
            for (uint32_t c = 0; c < 4; c++) {
                sum_a[c] += (pa >> (8 * c)) & 255u;
                sum_b[c] += (pb >> (8 * c)) & 255u;
            }
        }
}

// out5: max, mean, mean_squared, rms, psnr (the floats widened)
HOST_API void imh_reduce(const uint32_t* hist, uint32_t total_chans, uint32_t first_chan, uint32_t width, uint32_t height, int use_601, double* out5) {
    const bu::im_result r = bu::im_reduce(hist, total_chans, first_chan, width, height, use_601 != 0);
    out5[0] = r.max; out5[1] = r.mean; out5[2] = r.mean_squared; out5[3] = r.rms; out5[4] = r.psnr;
}
