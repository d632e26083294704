// etc1s_bc1.h -- ETC1S -> BC1 (convert_etc1s_to_dxt1, transcoder/basisu_transcoder.cpp:2271-2461), included by etc1s_transcode_kernels.hip in front of the families' target
// headers. One conversion for the plain BC1 target of every family and for FXT1, which is made of two BC1-like halves (etc1s_vendor_format_targets.h).
#pragma once

namespace bu {

// ---- BC1 (convert_etc1s_to_dxt1). THREE_COLOUR: the reference's use_threecolor_blocks. Plain BC1 passes true and a block with equal endpoints keeps them; FXT1 passes
// false, and such a block gets endpoints that differ by one, so that it can never be read as a three-colour block (:2289 and :2422).
template <bool THREE_COLOUR>
__device__ __forceinline__ uint2 to_bc1(const etc1s_entry& e, uint32_t sel, const uint32_t* endpoints5, const uint32_t* endpoints6) {
    uint32_t used = 0;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) used |= 1u << ((sel >> (2u * p)) & 3u);
    const uint32_t low = (uint32_t)__ffs((int)used) - 1u, high = 31u - (uint32_t)__clz((int)used);
    uint32_t colors[4];
    block_colors(e, colors);
    if (low == high) {   // one colour: the pair whose colour 1 is nearest, selectors all 2 (= colour 1 when low > high)
        const uint32_t c = pick4(colors, low), r = c & 255u, g = (c >> 8) & 255u, b = c >> 16;
        uint32_t max16 = ((uint32_t)ke_bc1_solid5[r * 2] << 11) | ((uint32_t)ke_bc1_solid6[g * 2] << 5) | ke_bc1_solid5[b * 2];
        uint32_t min16 = ((uint32_t)ke_bc1_solid5[r * 2 + 1] << 11) | ((uint32_t)ke_bc1_solid6[g * 2 + 1] << 5) | ke_bc1_solid5[b * 2 + 1];
        uint32_t mask = 0xAAu;
        if (!THREE_COLOUR && min16 == max16) {
            mask = 0u;
            if (min16 > 0) min16--;
            else { max16 = 1; min16 = 0; mask = 0x55u; }
        }
        if (max16 < min16) { const uint32_t t = max16; max16 = min16; min16 = t; mask ^= 0x55u; }
        return make_uint2(max16 | (min16 << 16), mask * 0x01010101u);
    }
    if (e.table >= 7 && __popc(used) == 2 && low == 0 && high == 3) {   // the widest table with only its extremes in use: the two colours become the endpoints
        const uint32_t c0 = colors[0], c3 = colors[3];
        uint32_t max16 = ((uint32_t)ke_bc1_end5[c0 & 255u] << 11) | ((uint32_t)ke_bc1_end6[(c0 >> 8) & 255u] << 5) | ke_bc1_end5[c0 >> 16];
        uint32_t min16 = ((uint32_t)ke_bc1_end5[c3 & 255u] << 11) | ((uint32_t)ke_bc1_end6[(c3 >> 8) & 255u] << 5) | ke_bc1_end5[c3 >> 16];
        uint32_t l = 0, h = 1;
        if (min16 == max16) {
            if (min16 > 0) { min16--; l = 0; h = 0; }
            else { max16 = 1; min16 = 0; l = 1; h = 1; }
        }
        if (max16 < min16) { const uint32_t t = max16; max16 = min16; min16 = t; l = 1; h = 0; }
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t p = 0; p < 16; p++) bits |= ((((sel >> (2u * p)) & 3u) == 3u) ? h : l) << (2u * p);
        return make_uint2(max16 | (min16 << 16), bits);
    }
    // per channel the best endpoints for each of the ten selector mappings; the mapping with the least summed error wins, first on ties
    const uint32_t range = ke_bc1_range_index[low * 4 + high];
    const uint32_t* tr = &endpoints5[((e.table * 32u + e.r5) * 6u + range) * 10u];
    const uint32_t* tg = &endpoints6[((e.table * 32u + e.g5) * 6u + range) * 10u];
    const uint32_t* tb = &endpoints5[((e.table * 32u + e.b5) * 6u + range) * 10u];
    uint32_t best_err = 0xFFFFFFFFu, best = 0, br = 0, bg = 0, bb = 0;
#pragma unroll
    for (uint32_t m = 0; m < 10; m++) {
        const uint32_t r = tr[m], g = tg[m], b = tb[m], err = (r >> 16) + (g >> 16) + (b >> 16);
        if (err < best_err) { best_err = err; best = m; br = r; bg = g; bb = b; }
    }
    uint32_t l = ((br & 255u) << 11) | ((bg & 255u) << 5) | (bb & 255u);
    uint32_t h = (((br >> 8) & 255u) << 11) | (((bg >> 8) & 255u) << 5) | ((bb >> 8) & 255u);
    uint32_t swapped = 0;
    if (l < h) { const uint32_t t = l; l = h; h = t; swapped = 1; }
    if (l == h) {
        if (THREE_COLOUR) return make_uint2(l | (h << 16), 0u);
        if (h > 0) return make_uint2(l | ((h - 1u) << 16), 0u);
        return make_uint2(1u, 0x55555555u);
    }
    const unsigned char* xl = &ke_bc1_selector_xlat[(best * 2u + swapped) * 4u];
    const uint32_t x0 = xl[0], x1 = xl[1], x2 = xl[2], x3 = xl[3];
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) {
        const uint32_t s = (sel >> (2u * p)) & 3u;
        bits |= ((s & 2u) ? ((s & 1u) ? x3 : x2) : ((s & 1u) ? x1 : x0)) << (2u * p);
    }
    return make_uint2(l | (h << 16), bits);
}

}  // namespace bu
