// Test-only host build of basis_universal_amd/csrc/texture_unpack.h (g++): the same texel functions the kernels run, called sixteen times per block.
#include "../../basis_universal_amd/csrc/texture_unpack.h"
#include "host_api.h"

using namespace bu_unpack;

HOST_API uint32_t th_bytes_per_block(uint32_t format) { return texture_bytes_per_block(format); }

// n blocks of `format` (transcoder_texture_format value; every format but PVRTC1) -> out (n, 64) texels, ok (n,) flags; returns 0 for a format that is not decoded
// block by block
HOST_API uint32_t th_unpack(const uint8_t* blocks, uint32_t n, uint32_t format, uint8_t* out, uint8_t* ok) {
    const uint32_t unit = texture_bytes_per_block(format);
    if (!unit || texture_format_is_pvrtc1(format)) return 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* b = blocks + (size_t)i * unit;
        uint8_t* o = out + (size_t)i * 64;
        bool r = false;
        switch (format) {
        case UF_ETC1: r = unpack_texture_block<UF_ETC1>(b, o); break;
        case UF_ETC2_RGBA: r = unpack_texture_block<UF_ETC2_RGBA>(b, o); break;
        case UF_EAC_R11: r = unpack_texture_block<UF_EAC_R11>(b, o); break;
        case UF_EAC_RG11: r = unpack_texture_block<UF_EAC_RG11>(b, o); break;
        case UF_ASTC_4x4: r = unpack_texture_block<UF_ASTC_4x4>(b, o); break;
        case UF_BC1: r = unpack_texture_block<UF_BC1>(b, o); break;
        case UF_BC3: r = unpack_texture_block<UF_BC3>(b, o); break;
        case UF_BC4: r = unpack_texture_block<UF_BC4>(b, o); break;
        case UF_BC5: r = unpack_texture_block<UF_BC5>(b, o); break;
        default: r = unpack_texture_block<UF_BC7>(b, o); break;
        }
        ok[i] = r ? 1 : 0;
    }
    return 1;
}

// a PVRTC1 image of nbx x nby blocks (powers of two) in Morton order -> out (nby * nbx, 64): the texels of block (bx, by) at index by * nbx + bx
HOST_API uint32_t th_unpack_pvrtc1(const uint8_t* blocks, uint32_t nbx, uint32_t nby, uint8_t* out) {
    if (!nbx || !nby || (nbx & (nbx - 1)) || (nby & (nby - 1))) return 0;
    for (uint32_t by = 0; by < nby; by++)
        for (uint32_t bx = 0; bx < nbx; bx++) unpack_pvrtc1_block(blocks, nbx, nby, bx, by, out + ((size_t)by * nbx + bx) * 64);
    return 1;
}

// BISE on its own, for the tests of the trit and quint groups: value k of a sequence of `values` values packed from bit 0 of 16 bytes -> m | tq << 8
HOST_API uint32_t th_ise_value(const uint8_t* bits16, uint32_t kind, uint32_t n, uint32_t values, uint32_t k) {
    uint64_t lo = load64(bits16), hi = load64(bits16 + 8);
    astc_window(lo, hi, 0, ise_sequence_bits(kind, n, values));
    uint32_t tq;
    const uint32_t m = ise_value(lo, hi, kind, n, k, &tq);
    return m | (tq << 8);
}
