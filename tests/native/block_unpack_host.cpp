// Test-only host build of basis_universal_amd/csrc/block_unpack.h (g++): the same texel functions the kernel runs, called sixteen times per block.
#include "../../basis_universal_amd/csrc/block_unpack.h"
#include "host_api.h"

using namespace bu_unpack;

// n blocks of `format` (transcoder_texture_format value) -> out (n, 64) texels, ok (n,) flags; returns 0 for a format that does not unpack here
HOST_API uint32_t bh_unpack(const uint8_t* blocks, uint32_t n, uint32_t format, uint8_t* out, uint8_t* ok) {
    const uint32_t unit = unpack_bytes_per_block(format);
    if (!unit) return 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* b = blocks + (size_t)i * unit;
        uint8_t* o = out + (size_t)i * 64;
        bool r = false;
        switch (format) {
        case UF_BC1: r = unpack_block_bc1(b, o); break;
        case UF_BC3: r = unpack_block_bc3(b, o); break;
        case UF_BC4: r = unpack_block_bc4(b, o); break;
        case UF_BC5: r = unpack_block_bc5(b, o); break;
        default: r = unpack_block_bc7(b, o); break;
        }
        ok[i] = r ? 1 : 0;
    }
    return 1;
}

// BC1's colour decode in forced four-colour mode (BC3's colour half), for the plumbing identities
HOST_API void bh_bc1_four(const uint8_t* blocks, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t v = load64(blocks + (size_t)i * 8);
        for (uint32_t t = 0; t < 16; t++) {
            const uint32_t px = unpack_texel_bc1(v, t, true);
            for (uint32_t k = 0; k < 4; k++) out[(size_t)i * 64 + t * 4 + k] = (uint8_t)(px >> (8 * k));
        }
    }
}
