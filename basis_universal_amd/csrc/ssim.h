// ssim.h -- compute_ssim of the reference (encoder/basisu_ssim.cpp, called from basisu_tool.cpp's -compare_ssim), stated once for the kernels (ssim_kernels.hip), the
// host library (host/ssim.cpp) and the native test (tests/native/ssim_host.cpp). Plain C++: compiles with and without hipcc. Build with -ffp-contract=off: every
// operation below is one separately rounded binary32 operation, as in the reference's x86-64 build (no FMA), and nothing here may fuse.
//
// One call compares two RGBA8 images of one size w x h (the caller crops to min(widths) x min(heights) first). With luma set every pixel becomes (Y, Y, Y, A), Y the
// integer 709 / 601 luma of image_metrics.h; then every channel is a float on the 0..255 scale. Per channel five images are filtered with one 11x11 Gaussian
// (sigma^2 = 2.25, weights normalised to sum 1): a, b, a*a, b*b, a*b (the three products are exact in binary32: at most 65025). The filter is a 121-term running sum
// c <- c + p * w from c = 0, rows (yd = -5..5) outer, columns (xd = -5..5) inner, coordinates clamped to the image. From the five filtered values
//      mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2,   s1_sq = F(a*a) - mu1_sq, s2_sq = F(b*b) - mu2_sq, s12 = F(a*b) - mu1_mu2,
//      t3 = (2 mu1_mu2 + C1) (2 s12 + C2),   t1 = (mu1_sq + mu2_sq + C1) (s1_sq + s2_sq + C2),   smap = t1 == 0 ? 0 : t3 / t1,    C1 = 6.5025f, C2 = 58.5225f
// and the figure of a channel is the mean of smap: ONE running binary32 sum over the pixels in raster order from 0, then one division by float(w * h).
//
// The reference writes the three subtractions as add_weighted_image: s * 1 + m * (-1) + 0. s * 1 = s and m * (-1) = -m exactly, so this is (s - m) + 0, which differs
// from s - m only where s - m is -0. It never is: every filtered value is a sum of non-negative products from +0, hence >= +0, so is every m, and in round-to-nearest
// x - y of two values >= +0 is -0 only for x = -0. (2 x + 0) + C and (x * y) * 1 are the plain expressions for the same reason or exactly.
//
// The running sum is the reference's behaviour and part of what it prints: at 256 x 192 the state's ulp is already 2^-8 while the addends are below 1, so the sixth
// decimal depends on the order. From 2^24 pixels on, an identical pair (every addend 1.0f) stops at 16777216: the mean then prints below 1.000000. Reproduced, not fixed.
#pragma once
#include <math.h>
#include <stdint.h>
#include "image_metrics.h"

#if defined(__HIPCC__)
#define BU_SSIM_HD __host__ __device__ __forceinline__
#define BU_SSIM_UNROLL _Pragma("unroll")
#define BU_SSIM_NO_UNROLL _Pragma("unroll 1")
#else
#define BU_SSIM_HD inline
#define BU_SSIM_UNROLL
#define BU_SSIM_NO_UNROLL
#endif

namespace bu {

enum : uint32_t { SSIM_RGBA = 0, SSIM_LUMA_709 = 1, SSIM_LUMA_601 = 2, SSIM_MODES = 3 };
enum : int { SSIM_RADIUS = 5, SSIM_TAPS = 11, SSIM_WEIGHTS = 121 };
// the planes of smap values one image pair has: the four channels of the RGBA call, channel 0 of the 709 call, channel 0 of the 601 call
enum : uint32_t { SSIM_PLANE_R = 0, SSIM_PLANE_G = 1, SSIM_PLANE_B = 2, SSIM_PLANE_A = 3, SSIM_PLANE_709 = 4, SSIM_PLANE_601 = 5, SSIM_PLANES = 6 };

struct ssim_weights { float w[SSIM_WEIGHTS]; };   // w[(yd + 5) * 11 + (xd + 5)]

// compute_gaussian_kernel(11, 11, 2.25f, normalize) in its own order: gauss() with expf / sqrtf for the first quadrant and the axes, the other three quadrants copied,
// the sum a double accumulated x outer and y inner, one_over_sum a double division, every weight float(w * one_over_sum). Host only (expf is libm's).
inline void ssim_gaussian_weights(float out[SSIM_WEIGHTS]) {
    const int n = SSIM_TAPS, mid = SSIM_RADIUS;
    const float sigma_sqr = 1.5f * 1.5f;
    double sum = 0;
    for (int x = 0; x < n; x++)
        for (int y = 0; y < n; y++) {
            float g;
            if (x > mid && y < mid) g = out[(n - x - 1) + y * n];
            else if (x < mid && y > mid) g = out[x + (n - y - 1) * n];
            else if (x > mid && y > mid) g = out[(n - x - 1) + (n - y - 1) * n];
            else {
                const int dx = x - mid, dy = y - mid;
                const float e = expf(-((dx * dx + dy * dy) / (2.0f * sigma_sqr)));
                g = (1.0f / (sqrtf((float)(2.0f * 3.14159265358979323846 * sigma_sqr)))) * e;
            }
            out[x + y * n] = g;
            sum += g;
        }
    const double one_over_sum = 1.0f / sum;
    for (int i = 0; i < n * n; i++) out[i] = static_cast<float>(out[i] * one_over_sum);
}

// What a pixel (r | g << 8 | b << 16 | a << 24) contributes to a call, one byte per channel computed. C = 4: the RGBA call, the pixel itself. C = 2: channel 0 of BOTH
// luma calls side by side (709 in byte 0, 601 in byte 1); channels 1-3 of a luma call are never printed and never computed.
template <int C> BU_SSIM_HD uint32_t ssim_sample(uint32_t px) {
    if (C == 4) return px;
    const int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
    return (uint32_t)im_luma_709(r, g, b) | ((uint32_t)im_luma_601(r, g, b) << 8);
}

template <int C> struct ssim_acc { float a[C], b[C], aa[C], bb[C], ab[C]; };

template <int C> BU_SSIM_HD void ssim_clear(ssim_acc<C>& s) {
    BU_SSIM_UNROLL
    for (int c = 0; c < C; c++) s.a[c] = s.b[c] = s.aa[c] = s.bb[c] = s.ab[c] = 0.0f;
}

// one tap of the five filters of every channel: c <- c + p * w, the product rounded before the add
template <int C> BU_SSIM_HD void ssim_tap(ssim_acc<C>& s, uint32_t sa, uint32_t sb, float w) {
    BU_SSIM_UNROLL
    for (int c = 0; c < C; c++) {
        const float a = (float)((sa >> (8 * c)) & 255u), b = (float)((sb >> (8 * c)) & 255u);
        s.a[c] = s.a[c] + a * w;
        s.b[c] = s.b[c] + b * w;
        s.aa[c] = s.aa[c] + (a * a) * w;
        s.bb[c] = s.bb[c] + (b * b) * w;
        s.ab[c] = s.ab[c] + (a * b) * w;
    }
}

BU_SSIM_HD float ssim_div(float x, float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(x, y);
#else
    return x / y;
#endif
}

// the five filtered values of one channel -> its smap value
BU_SSIM_HD float ssim_value(float mu1, float mu2, float f_aa, float f_bb, float f_ab) {
    const float C1 = 6.50250f, C2 = 58.52250f;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float s1_sq = (f_aa * 1.0f + mu1_sq * -1.0f) + 0.0f;
    const float s2_sq = (f_bb * 1.0f + mu2_sq * -1.0f) + 0.0f;
    const float s12 = (f_ab * 1.0f + mu1_mu2 * -1.0f) + 0.0f;
    const float t3 = ((2.0f * mu1_mu2 + 0.0f) + C1) * ((2.0f * s12 + 0.0f) + C2);
    const float t1 = ((mu1_sq + mu2_sq) + C1) * ((s1_sq + s2_sq) + C2);
    return t1 == 0.0f ? 0.0f : ssim_div(t3, t1);
}

// The C smap values of one output pixel. at(xd, yd, sa, sb) hands over the two samples (ssim_sample) at the pixel's offset -5..5 each way, already clamped to the
// image; the taps are walked in the reference's order, rows outer.
template <int C, class At> BU_SSIM_HD void ssim_pixel(const At& at, const ssim_weights& k, float out[C]) {
    ssim_acc<C> s;
    ssim_clear(s);
    BU_SSIM_NO_UNROLL
    for (int yd = -SSIM_RADIUS; yd <= SSIM_RADIUS; yd++) {
        BU_SSIM_UNROLL
        for (int xd = -SSIM_RADIUS; xd <= SSIM_RADIUS; xd++) {
            uint32_t sa, sb;
            at(xd, yd, sa, sb);
            ssim_tap(s, sa, sb, k.w[(yd + SSIM_RADIUS) * SSIM_TAPS + (xd + SSIM_RADIUS)]);
        }
    }
    BU_SSIM_UNROLL
    for (int c = 0; c < C; c++) out[c] = ssim_value(s.a[c], s.b[c], s.aa[c], s.bb[c], s.ab[c]);
}

// avg_image for one channel: the plain serial form the host restatement uses
inline float ssim_avg(const float* v, uint64_t n) {
    float s = 0.0f;
    for (uint64_t i = 0; i < n; i++) s = s + v[i];
    return s / static_cast<float>(n);
}

}  // namespace bu
