// Test-only host build of basis_universal_amd/csrc/source_prep.h (g++): the same per-pixel functions the kernels run, in serial loops.
#include "../../basis_universal_amd/csrc/source_prep.h"
#include "host_api.h"
#include <stddef.h>

// image::renormalize_normal_map over n pixels (r | g << 8 | b << 16 | a << 24), in place
HOST_API void sph_renormalize(uint32_t* px, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) px[i] = bu::renormalize_pixel(px[i]);
}

// the whole preparation of a w x h image, pitches in pixels; src and dst must not overlap. flags[0] = has_alpha, flags[1] = any prepared alpha below 255.
// Returns 0 for a swizzle entry above 3.
HOST_API uint32_t sph_prepare(const uint32_t* src, uint32_t w, uint32_t h, uint32_t src_pitch, uint32_t* dst, uint32_t dst_pitch, uint32_t renormalize, uint32_t swizzle,
                              uint32_t check_for_alpha, uint32_t force_alpha, uint32_t y_flip, uint32_t* flags) {
    if (!bu::source_prep_swizzle_valid(swizzle)) return 0;
    const bu::source_prep_options o = { renormalize, swizzle, check_for_alpha, force_alpha, y_flip };
    const bool opaque = bu::source_prep_alpha_opaque(o);
    bool below = false;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint32_t v = bu::prepare_pixel(src[(size_t)bu::source_row(y, h, y_flip != 0) * src_pitch + x], renormalize != 0, swizzle, opaque);
            below |= (v >> 24) < 255u;
            dst[(size_t)y * dst_pitch + x] = v;
        }
    flags[0] = bu::source_prep_has_alpha(o, below) ? 1u : 0u;
    flags[1] = below ? 1u : 0u;
    return 1;
}

HOST_API void sph_split_alpha(const uint32_t* src, uint64_t n, uint32_t* rgb, uint32_t* alpha) {
    for (uint64_t i = 0; i < n; i++) { rgb[i] = bu::split_alpha_rgb(src[i]); alpha[i] = bu::split_alpha_a(src[i]); }
}
