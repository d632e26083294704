// dds_pack.h -- the payload of a DX10 .dds file, per 4x4 tile and per pixel: what the reference tool's `-dds` mode makes of a prepared slice image
// (pack_slice / pack_uncompressed_pixel, encoder/basisu_dds_export.cpp:151-267) for BC1-BC5 and the seven uncompressed formats.
//   bc1 = basist::encode_bc1(cEncodeBC1HighQuality) = bc1_encode(px, false, 0, 2) of uastc_core.h (two least-squares passes; solid tiles through bc1_solid)
//   bc2 = four little-endian 16-bit rows of a >> 4 (texel x at nibble x), then the bc1 block
//   bc3 = bc4_encode(px, 3) (uastc_transcode.h), then the bc1 block;  bc4 = bc4_encode(px, 0);  bc5 = bc4_encode(px, 0), bc4_encode(px, 1)
//   raw : the channels truncated to the format's bits, never rounded (r >> 3, a >= 128, a >> 4): the inverse of a reader's bit replication
// A tile is 16 packed texels (r | g << 8 | b << 16 | a << 24: the resident tile array's bytes as little-endian words) held in registers; nothing is indexed by a
// run-time value. BC7 is not here: neither of the reference's two BC7 packers (bc7f, bc7e_scalar) is restated in this package.
// Same convention as uastc_core.h: hipcc compiles it for dds_pack_kernels.hip, g++ for the test-only host library (tests/native/dds_pack_host.cpp).
#pragma once
#include "uastc_transcode.h"

namespace bu_dds {
using namespace bu_uastc;

// the reference's dds_output_format values (basisu_dds_export.h): the order of the tool's -dds_format tokens
enum { FMT_BC1 = 0, FMT_BC2 = 1, FMT_BC3 = 2, FMT_BC4 = 3, FMT_BC5 = 4, FMT_BC7 = 5, FMT_A8R8G8B8 = 6, FMT_A8B8G8R8 = 7, FMT_R8 = 8, FMT_R8G8 = 9, FMT_R5G6B5 = 10,
       FMT_A1R5G5B5 = 11, FMT_A4R4G4B4 = 12, FMT_TOTAL = 13 };

BU_FN_HD bool is_block_format(uint32_t fmt) { return fmt <= FMT_BC5; }                           // BC7 is refused by every caller
BU_FN_HD bool is_pixel_format(uint32_t fmt) { return fmt >= FMT_A8R8G8B8 && fmt < FMT_TOTAL; }
// bytes per 4x4 block of a block format, bytes per pixel of a raw one; 0: BC7 or not a format
BU_FN_HD uint32_t unit_bytes(uint32_t fmt) {
    switch (fmt) {
    case FMT_BC1: case FMT_BC4: return 8;
    case FMT_BC2: case FMT_BC3: case FMT_BC5: return 16;
    case FMT_A8R8G8B8: case FMT_A8B8G8R8: return 4;
    case FMT_R8: return 1;
    case FMT_R8G8: case FMT_R5G6B5: case FMT_A1R5G5B5: case FMT_A4R4G4B4: return 2;
    default: return 0;
    }
}

// BC2's explicit alpha: row y is bits 16 y .. 16 y + 15, texel x its nibble x
BU_FN uint64_t bc2_alpha(const uint32_t* px) {
    uint64_t out = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) out |= (uint64_t)(px[i] >> 28) << (4 * i);
    return out;
}

// One tile -> out[0] (the first 8 bytes, little-endian) and, for the 16-byte formats, out[1]. fmt: a block format other than BC7.
BU_FN void pack_block(const uint32_t* px, uint32_t fmt, uint64_t* out) {
    if (fmt == FMT_BC1) out[0] = bc1_bits(bc1_encode(px, false, 0, 2));
    else if (fmt == FMT_BC2) { out[0] = bc2_alpha(px); out[1] = bc1_bits(bc1_encode(px, false, 0, 2)); }
    else if (fmt == FMT_BC3) { out[0] = bc4_encode(px, 3); out[1] = bc1_bits(bc1_encode(px, false, 0, 2)); }
    else if (fmt == FMT_BC4) out[0] = bc4_encode(px, 0);
    else { out[0] = bc4_encode(px, 0); out[1] = bc4_encode(px, 1); }
}

// One texel -> the low unit_bytes(fmt) bytes of the result, little-endian. fmt: a raw format.
BU_FN uint32_t pack_pixel(uint32_t p, uint32_t fmt) {
    const uint32_t r = p & 255u, g = (p >> 8) & 255u, b = (p >> 16) & 255u, a = p >> 24;
    switch (fmt) {
    case FMT_A8R8G8B8: return b | (g << 8) | (r << 16) | (a << 24);   // DXGI B8G8R8A8: memory order B, G, R, A
    case FMT_A8B8G8R8: return p;                                      // DXGI R8G8B8A8
    case FMT_R8: return r;
    case FMT_R8G8: return r | (g << 8);
    case FMT_R5G6B5: return ((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3);
    case FMT_A1R5G5B5: return (a >= 128u ? 0x8000u : 0u) | ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3);
    default: return ((a >> 4) << 12) | ((r >> 4) << 8) | ((g >> 4) << 4) | (b >> 4);   // FMT_A4R4G4B4
    }
}

}  // namespace bu_dds
