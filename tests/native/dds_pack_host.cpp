// Test-only host build of the DDS payload packers (basis_universal_amd/csrc/dds_pack.h): the same per-tile and per-pixel functions the HIP kernels run, compiled by
// g++ so that the CPU suite can hold every block of every golden .dds payload to the reference tool's bytes without a GPU.
#include <string.h>
#include "../../basis_universal_amd/csrc/dds_pack.h"
#include "host_api.h"

using namespace bu_dds;

HOST_API uint32_t hd_unit_bytes(uint32_t fmt) { return unit_bytes(fmt); }
HOST_API uint32_t hd_is_block_format(uint32_t fmt) { return is_block_format(fmt) ? 1u : 0u; }

// n tiles of 64 bytes (16 RGBA texels, rows of four) -> n blocks of unit_bytes(fmt); returns 0 for a format that is no block format
HOST_API uint32_t hd_pack_blocks(const uint8_t* tiles, uint32_t n, uint32_t fmt, uint8_t* out) {
    if (!is_block_format(fmt)) return 0;
    const uint32_t unit = unit_bytes(fmt);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t px[16];
        for (int k = 0; k < 16; k++) px[k] = pack_px(tiles + (size_t)i * 64 + k * 4);
        uint64_t w[2] = { 0, 0 };
        pack_block(px, fmt, w);
        memcpy(out + (size_t)i * unit, w, unit);
    }
    return 1;
}

// n RGBA texels -> n pixels of unit_bytes(fmt), little-endian; returns 0 for a format that is no raw format
HOST_API uint32_t hd_pack_pixels(const uint8_t* rgba, uint32_t n, uint32_t fmt, uint8_t* out) {
    if (!is_pixel_format(fmt)) return 0;
    const uint32_t unit = unit_bytes(fmt);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = pack_pixel(pack_px(rgba + (size_t)i * 4), fmt);
        memcpy(out + (size_t)i * unit, &v, unit);
    }
    return 1;
}
