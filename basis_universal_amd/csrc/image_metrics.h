// image_metrics.h -- image_metrics::calc of the reference (encoder/basisu_enc.cpp:2155-2226), stated once for the kernel (image_metrics_kernels.hip), the host library
// (host/image_metrics.cpp) and the native test (tests/native/image_metrics_host.cpp). Plain C++: compiles with and without hipcc.
//
// calc is integer work under a thin layer of doubles: a 256-bin histogram of |a - b| over the chosen channels (or of the luma difference), then sum i * h[i] and
// sum i * i * h[i] in ascending bin order. The histogram is a set of integer counts, so whoever counts -- in whatever order -- gets the reference's bins exactly; the
// doubles start at the bins (im_reduce below, the reference's own expression order).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BU_IM_HD __host__ __device__ inline
#else
#define BU_IM_HD inline
#endif

namespace bu {

enum : uint32_t { IM_R = 0, IM_G = 1, IM_B = 2, IM_A = 3, IM_LUMA_709 = 4, IM_LUMA_601 = 5, IM_ROWS = 6, IM_BINS = 256 };

// color_rgba::get_709_luma / get_601_luma (enc.h:1051-1052): per image, then differenced
BU_IM_HD int im_luma_709(int r, int g, int b) { return (13938 * r + 46869 * g + 4729 * b + 32768) >> 16; }
BU_IM_HD int im_luma_601(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
BU_IM_HD uint32_t im_abs_diff(int a, int b) { return (uint32_t)(a > b ? a - b : b - a); }

// the six bins one pixel pair lands in (rows IM_R .. IM_LUMA_601); pa / pb: r | g << 8 | b << 16 | a << 24
BU_IM_HD void im_pixel_bins(uint32_t pa, uint32_t pb, uint32_t bins[IM_ROWS]) {
    const int ra = pa & 255, ga = (pa >> 8) & 255, ba = (pa >> 16) & 255, aa = pa >> 24;
    const int rb = pb & 255, gb = (pb >> 8) & 255, bb = (pb >> 16) & 255, ab = pb >> 24;
    bins[IM_R] = im_abs_diff(ra, rb);
    bins[IM_G] = im_abs_diff(ga, gb);
    bins[IM_B] = im_abs_diff(ba, bb);
    bins[IM_A] = im_abs_diff(aa, ab);
    bins[IM_LUMA_709] = im_abs_diff(im_luma_709(ra, ga, ba), im_luma_709(rb, gb, bb));
    bins[IM_LUMA_601] = im_abs_diff(im_luma_601(ra, ga, ba), im_luma_601(rb, gb, bb));
}

struct im_result { double max; float mean, mean_squared, rms, psnr; };

// hist[IM_ROWS][IM_BINS] -> what calc(a, b, first_chan, total_chans, avg_comp_error = true, use_601) leaves in m_max / m_mean / m_mean_squared / m_rms / m_psnr.
// total_chans 1..4: the sum of the channel rows first_chan .. first_chan + total_chans - 1 (calc counts them into one histogram); 0: a luma row. A bin of the
// reference is a double that was incremented by one per value, so it holds the integer count exactly (counts stay below 2^53), as the sum of the rows does here.
inline im_result im_reduce(const uint32_t* hist, uint32_t total_chans, uint32_t first_chan, uint32_t width, uint32_t height, bool use_601) {
    im_result r;
    r.max = 0;
    double sum = 0.0f, sum2 = 0.0f;
    for (uint32_t i = 0; i < IM_BINS; i++) {
        double h = 0;
        if (total_chans) {
            for (uint32_t c = 0; c < total_chans; c++) h += (double)hist[(first_chan + c) * IM_BINS + i];
        } else
            h = (double)hist[(use_601 ? IM_LUMA_601 : IM_LUMA_709) * IM_BINS + i];
        if (h) {
            r.max = r.max > (double)i ? r.max : (double)i;
            double v = i * h;
            sum += v;
            sum2 += i * v;
        }
    }
    double total_values = (double)width * (double)height;
    const uint32_t chans = total_chans < 1 ? 1 : (total_chans > 4 ? 4 : total_chans);
    total_values *= (double)chans;
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    r.mean = (float)clampd(sum / total_values, 0.0f, 255.0);
    r.mean_squared = (float)clampd(sum2 / total_values, 0.0f, 255.0f * 255.0f);
    r.rms = (float)sqrt((double)r.mean_squared);
    r.psnr = r.rms ? (float)clampd(log10(255.0 / (double)r.rms) * 20.0f, 0.0f, 100.0f) : 100.0f;
    return r;
}

}  // namespace bu
