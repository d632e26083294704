// Test-only host build of the UASTC texture family's further targets (the second half of basis_universal_amd/csrc/uastc_transcode.h): ETC1, ETC2 RGBA, EAC R11 /
// RG11 and the 16-bit pixel formats, the same functions the HIP kernel runs, compiled by g++. ht_texture is every target of the family behind one entry (the first
// family's seven through the functions tests/native/transcode_host.cpp calls); the rest expose the pieces the tests look at on their own.
#include <string.h>
#include "../../basis_universal_amd/csrc/uastc_transcode.h"
#include "host_api.h"

using namespace bu_uastc;

template <uint32_t TARGET>
static bool etc_block(const uint8_t* blk, bool hq, uint32_t c0, uint32_t c1, uint64_t* w) {
    return hq ? transcode_etc<TARGET, true>(blk, c0, c1, w) : transcode_etc<TARGET, false>(blk, c0, c1, w);
}

// One block of any target of the family into `out` (texture_unit_bytes per block; pixel targets: the 16 texels in raster order, 64 or 32 bytes). A refused block
// is zero-filled, as the kernel leaves it.
static bool texture_block(const uint8_t* blk, uint32_t target, bool hq, uint32_t c0, uint32_t c1, uint8_t* out) {
    uint64_t w[2] = { 0, 0 };
    bool ok;
    switch (target) {
    case TF_RGBA32: case TF_RGB565: case TF_BGR565: case TF_RGBA4444: {
        rgba8 px[16];
        ok = transcode_rgba32(blk, px);
        if (target == TF_RGBA32) { if (ok) memcpy(out, px, 64); else memset(out, 0, 64); return ok; }
        for (int i = 0; i < 16; i++) {
            const uint32_t v = !ok ? 0u : (target == TF_RGB565 ? pack_pixel16<TF_RGB565>(px[i]) : (target == TF_BGR565 ? pack_pixel16<TF_BGR565>(px[i]) : pack_pixel16<TF_RGBA4444>(px[i])));
            out[2 * i] = (uint8_t)v; out[2 * i + 1] = (uint8_t)(v >> 8);
        }
        return ok;
    }
    case TF_ASTC_4x4_RGBA: case TF_BC7_RGBA:
        ok = target == TF_BC7_RGBA ? transcode_bc7(blk, out) : transcode_astc(blk, out);
        if (!ok) memset(out, 0, 16);
        return ok;
    case TF_ETC1_RGB: ok = etc_block<TF_ETC1_RGB>(blk, hq, c0, c1, w); break;
    case TF_ETC2_RGBA: ok = etc_block<TF_ETC2_RGBA>(blk, hq, c0, c1, w); break;
    case TF_ETC2_EAC_R11: ok = etc_block<TF_ETC2_EAC_R11>(blk, hq, c0, c1, w); break;
    case TF_ETC2_EAC_RG11: ok = etc_block<TF_ETC2_EAC_RG11>(blk, hq, c0, c1, w); break;
    default: ok = transcode_bcn(blk, target, hq, c0, c1, w); break;
    }
    if (!ok) w[0] = w[1] = 0;
    memcpy(out, w, texture_unit_bytes(target));
    return ok;
}

// bytes per block ht_texture writes for `target`; 0 = not a target of the family
HOST_API uint32_t ht_texture_block_bytes(uint32_t target) { return texture_unit_bytes(target) * (texture_is_pixel_target(target) ? 16u : 1u); }

// n blocks -> n x ht_texture_block_bytes; returns the number of refused blocks, `ok` (may be null) one flag per block
HOST_API uint32_t ht_texture(const uint8_t* blocks, uint32_t n, uint32_t target, int high_quality, uint32_t chan0, uint32_t chan1, uint8_t* out, uint8_t* ok) {
    const uint32_t bytes = ht_texture_block_bytes(target);
    uint32_t bad = 0;
    if (!bytes) return n;
    for (uint32_t i = 0; i < n; i++) {
        const bool good = texture_block(blocks + (size_t)i * 16, target, high_quality != 0, chan0, chan1, out + (size_t)i * bytes);
        if (!good) bad++;
        if (ok) ok[i] = good ? 1 : 0;
    }
    return bad;
}

// pack_eac / pack_eac_high_quality of n x 16 raw values (raster order) -> n x 8 bytes
HOST_API void ht_pack_eac(const uint8_t* values, uint32_t n, int high_quality, uint8_t* out8) {
    for (uint32_t i = 0; i < n; i++) {
        int a[16];
        for (int k = 0; k < 16; k++) a[k] = values[(size_t)i * 16 + k];
        const uint64_t w = high_quality ? eac_pack<true>(a) : eac_pack<false>(a);
        memcpy(out8 + (size_t)i * 8, &w, 8);
    }
}

// the ETC hints of n blocks, 8 bytes each: [0] 0 refused, 1 solid, 2 any other; [1] flip, [2] diff, [3] inten0, [4] inten1, [5] bias, [6] the EAC byte,
// [7] 1 = the mode carries a bias | 2 = the mode has alpha. A solid block: [1] its selector, [3] its table.
HOST_API void ht_etc_hints(const uint8_t* blocks, uint32_t n, uint8_t* out8) {
    for (uint32_t i = 0; i < n; i++) {
        uint8_t* o = out8 + (size_t)i * 8;
        memset(o, 0, 8);
        cand c;
        if (!unpack_block(blocks + (size_t)i * 16, c)) continue;
        const etc_hints h = read_etc_hints(blocks + (size_t)i * 16, c.mode);
        o[0] = c.mode == 8 ? 1 : 2;
        o[1] = (uint8_t)(c.mode == 8 ? h.selector : h.flip); o[2] = (uint8_t)h.diff; o[3] = (uint8_t)h.inten0; o[4] = (uint8_t)h.inten1; o[5] = (uint8_t)h.bias; o[6] = (uint8_t)h.etc2;
        o[7] = (uint8_t)((ku_mode_has_etc1_bias[c.mode] ? 1 : 0) | (ku_mode_has_alpha[c.mode] ? 2 : 0));
    }
}
