// Test-only host build of the UASTC transcode core (basis_universal_amd/csrc/uastc_transcode.h): the same functions the HIP kernel runs, compiled by g++
// so that the CPU suite can diff every target against the reference's known answers. One C entry per target; each returns the number of blocks
// the core refused (their output is zero-filled, as the kernel leaves it) and, where `ok` is given, one flag per block.
#include <string.h>
#include "../../basis_universal_amd/csrc/uastc_transcode.h"

using namespace bu_uastc;

extern "C" {

uint32_t ht_rgba32(const uint8_t* blocks, uint32_t n, uint8_t* out64, uint8_t* ok) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        rgba8 px[16];
        const bool good = transcode_rgba32(blocks + (size_t)i * 16, px);
        if (good) memcpy(out64 + (size_t)i * 64, px, 64); else { memset(out64 + (size_t)i * 64, 0, 64); bad++; }
        if (ok) ok[i] = good ? 1 : 0;
    }
    return bad;
}

uint32_t ht_astc(const uint8_t* blocks, uint32_t n, uint8_t* out16, uint8_t* ok) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool good = transcode_astc(blocks + (size_t)i * 16, out16 + (size_t)i * 16);
        if (!good) { memset(out16 + (size_t)i * 16, 0, 16); bad++; }
        if (ok) ok[i] = good ? 1 : 0;
    }
    return bad;
}

uint32_t ht_bc7(const uint8_t* blocks, uint32_t n, uint8_t* out16, uint8_t* ok) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool good = transcode_bc7(blocks + (size_t)i * 16, out16 + (size_t)i * 16);
        if (!good) { memset(out16 + (size_t)i * 16, 0, 16); bad++; }
        if (ok) ok[i] = good ? 1 : 0;
    }
    return bad;
}

// target: TF_BC1_RGB, TF_BC3_RGBA, TF_BC4_R or TF_BC5_RG
uint32_t ht_bcn(const uint8_t* blocks, uint32_t n, uint32_t target, int high_quality, uint32_t chan0, uint32_t chan1, uint8_t* out, uint8_t* ok) {
    const uint32_t bytes = transcode_bytes_per_block(target);
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t w[2] = { 0, 0 };
        const bool good = transcode_bcn(blocks + (size_t)i * 16, target, high_quality != 0, chan0, chan1, w);
        if (!good) { w[0] = w[1] = 0; bad++; }
        memcpy(out + (size_t)i * bytes, w, bytes);
        if (ok) ok[i] = good ? 1 : 0;
    }
    return bad;
}

// the two BC1 hint bits of a block: 0 invalid / solid, otherwise 1 | hint0 << 1 | hint1 << 2
uint32_t ht_bc1_hints(const uint8_t* blk) {
    cand c;
    if (!unpack_block(blk, c) || c.mode == 8) return 0;
    bool h0, h1;
    read_bc1_hints(blk, c.mode, h0, h1);
    return 1u | (h0 ? 2u : 0u) | (h1 ? 4u : 0u);
}

uint32_t ht_mode(const uint8_t* blk) { cand c; return unpack_block(blk, c) ? c.mode : 255u; }

}
