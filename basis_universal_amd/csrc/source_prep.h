// source_prep.h -- what basis_compressor::read_source_images (encoder/basisu_comp.cpp:2569-2640) does to every pixel of a source image before the first block is cut,
// stated once for the kernels (source_prep_kernels.hip) and the native test (tests/native/source_prep_host.cpp). Plain C++: compiles with and without hipcc. Build with
// -ffp-contract=off: every float operation below is one separately rounded binary32 operation, as in the reference's x86-64 build, and nothing here may fuse.
//
// A pixel is one uint32: r | g << 8 | b << 16 | a << 24 (color_rgba in memory). The reference's order, which prepare_pixel keeps:
//   1. image::renormalize_normal_map (encoder/basisu_enc.h:3244-3283), with m_renormalize
//   2. the swizzle: set_noclamp_rgba(c[s0], c[s1], c[s2], c[s3])
//   3. the alpha policy (comp.cpp:2612-2625): forced alpha, or a swizzle with s3 != 3, keeps alpha and the image HAS alpha; otherwise without check_for_alpha alpha
//      becomes 255 and the image has none; otherwise alpha is kept and the image has alpha where any PREPARED alpha value is below 255
//   4. image::flip_y: only a row index (source_row), so one pass over the destination does all four
//
// renormalize_pixel, rule by rule:
//   (128, 128, 128) is left alone. v = float(c) * (2.0f / 255.0f) - 1.0f per component (the quotient is one binary32 constant; 255 maps just above 1), clamped to
//   [-1, 1]. length = sqrt((x*x + y*y) + z*z): vec::dot_product starts from the first product and adds the others in index order; sqrt of a binary32 value is
//   correctly rounded whether the reference's unqualified call resolves to the float or the double overload (53 >= 2 * 24 + 2 bits). length < .077f: the pixel becomes
//   (128, 128, 128, a). Otherwise, only where fabs(length - 1.0f) > .077f: every component is DIVIDED by length (vec::operator/=(T) divides; no reciprocal), then
//   c = clamp(floor((v + 1.0f) * 255.0f * .5f + .5f), 0, 255), left to right, and a result with r == 128 and g == 128 gets b = 0 below 128, else 255. Alpha is never touched.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BU_SP_HD __host__ __device__ __forceinline__
#else
#define BU_SP_HD inline
#endif

namespace bu {

enum : uint32_t { SOURCE_PREP_IDENTITY_SWIZZLE = 0x03020100u };   // s0 | s1 << 8 | s2 << 16 | s3 << 24: which source channel each destination channel takes

struct source_prep_options {
    uint32_t renormalize;      // m_renormalize
    uint32_t swizzle;          // packed as above, every entry 0..3
    uint32_t check_for_alpha;  // m_check_for_alpha
    uint32_t force_alpha;      // m_force_alpha
    uint32_t y_flip;           // m_y_flip
};

BU_SP_HD float source_prep_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // basisu::clamp

BU_SP_HD uint32_t source_prep_quantize(float v) {
    return (uint32_t)source_prep_clamp(floorf((v + 1.0f) * 255.0f * .5f + .5f), 0.0f, 255.0f);
}

BU_SP_HD uint32_t renormalize_pixel(uint32_t px) {
    const uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u, a = px & 0xFF000000u;
    if (r == 128u && g == 128u && b == 128u) return px;
    const float k = 2.0f / 255.0f, thresh = .077f;
    float x = source_prep_clamp((float)r * k - 1.0f, -1.0f, 1.0f);
    float y = source_prep_clamp((float)g * k - 1.0f, -1.0f, 1.0f);
    float z = source_prep_clamp((float)b * k - 1.0f, -1.0f, 1.0f);
    float norm = x * x;
    norm += y * y;
    norm += z * z;
    const float length = sqrtf(norm);
    if (length < thresh) return a | 0x808080u;
    if (!(fabsf(length - 1.0f) > thresh)) return px;
    x /= length; y /= length; z /= length;   // length >= .077f here: the reference's `if (length)` always holds
    const uint32_t nr = source_prep_quantize(x), ng = source_prep_quantize(y);
    uint32_t nb = source_prep_quantize(z);
    if (ng == 128u && nr == 128u) nb = nb < 128u ? 0u : 255u;
    return a | nr | (ng << 8) | (nb << 16);
}

BU_SP_HD uint32_t swizzle_pixel(uint32_t px, uint32_t swizzle) {
    const uint32_t c0 = (px >> (8u * (swizzle & 3u))) & 255u, c1 = (px >> (8u * ((swizzle >> 8) & 3u))) & 255u;
    const uint32_t c2 = (px >> (8u * ((swizzle >> 16) & 3u))) & 255u, c3 = (px >> (8u * ((swizzle >> 24) & 3u))) & 255u;
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

BU_SP_HD bool source_prep_swizzle_valid(uint32_t swizzle) { return (swizzle & 0xFCFCFCFCu) == 0u; }
BU_SP_HD bool source_prep_alpha_swizzled(uint32_t swizzle) { return (swizzle >> 24) != 3u; }
// the policy's two answers: is alpha overwritten with 255, and does the image have alpha given whether any prepared alpha value is below 255
BU_SP_HD bool source_prep_alpha_opaque(const source_prep_options& o) { return !o.force_alpha && !source_prep_alpha_swizzled(o.swizzle) && !o.check_for_alpha; }
BU_SP_HD bool source_prep_has_alpha(const source_prep_options& o, bool any_below_255) {
    if (o.force_alpha || source_prep_alpha_swizzled(o.swizzle)) return true;
    return o.check_for_alpha ? any_below_255 : false;
}

// steps 1-3 on one pixel; RENORM and the other two decisions are uniform over a launch
BU_SP_HD uint32_t prepare_pixel(uint32_t px, bool renormalize, uint32_t swizzle, bool opaque) {
    if (renormalize) px = renormalize_pixel(px);
    if (swizzle != SOURCE_PREP_IDENTITY_SWIZZLE) px = swizzle_pixel(px, swizzle);
    return opaque ? (px | 0xFF000000u) : px;
}

// step 4: the source row destination row y is made from
BU_SP_HD uint32_t source_row(uint32_t y, uint32_t height, bool y_flip) { return y_flip ? height - 1u - y : y; }

// the ETC1S alpha split (comp.cpp:2883-2903): a level with alpha becomes (r, g, b, 255) and (a, a, a, 255)
BU_SP_HD uint32_t split_alpha_rgb(uint32_t px) { return px | 0xFF000000u; }
BU_SP_HD uint32_t split_alpha_a(uint32_t px) { const uint32_t a = px >> 24; return a | (a << 8) | (a << 16) | 0xFF000000u; }

}  // namespace bu
