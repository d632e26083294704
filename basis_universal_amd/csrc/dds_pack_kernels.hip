// dds_pack_kernels.hip -- the payload of a DX10 .dds file from the resident tile array (dds_pack.h): one lane per 4x4 tile, the format a template parameter so that
// each instance carries only its own path. A tile is loaded as four 16-byte words, consecutive lanes on consecutive tiles.
//   k_dds_pack_blocks : BC1-BC5. The tile array is in slice order -- image outermost, then level -- which is DDS subresource order (layer, face, level), and a block
//                       format's subresource is its tiles in raster order: the whole file's payload is tile i -> out[i], one uint2 / uint4 store, no slice table.
//   k_dds_pack_pixels : the seven raw formats. Rows are tight (exactly width x height pixels per subresource), so a lane needs its slice: find_transcode_slice of
//                       tile_raster.h. A tile's row is cropped to the slice's width and stored by store_tile_row: one 16 / 8 / 4-byte word where it is whole and
//                       its address allows, else texel by texel; rows past the slice's height are not written.
#include <hip/hip_runtime.h>
#include "dds_pack.h"
#include "dds_pack_kernels.h"
#include "tile_raster.h"

namespace bu {
using namespace bu_dds;

__device__ __forceinline__ void load_tile(const uint4* __restrict__ t, uint32_t* px) {
    BU_UNROLL
    for (int y = 0; y < 4; y++) {
        const uint4 row = t[y];
        px[y * 4] = row.x; px[y * 4 + 1] = row.y; px[y * 4 + 2] = row.z; px[y * 4 + 3] = row.w;
    }
}

template <uint32_t FMT>
__global__ __launch_bounds__(256) void k_dds_pack_blocks(const uint4* __restrict__ tiles, void* __restrict__ out, uint32_t n_tiles) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_tiles) return;
    uint32_t px[16];
    load_tile(tiles + (size_t)i * 4, px);
    uint64_t w[2] = { 0, 0 };
    pack_block(px, FMT, w);
    store_block_words(out, i, w, !(FMT == FMT_BC1 || FMT == FMT_BC4));
}

struct dds_pixels_args {
    const uint4* tiles;
    uint8_t* out;
    const bu_hip_transcode_slice* slices;   // as the entry normalised them
    const uint32_t* prefix;
    uint32_t n_slices, total_tiles;
};

template <uint32_t FMT>
__global__ __launch_bounds__(256) void k_dds_pack_pixels(dds_pixels_args a) {
    transcode_slice_view v;
    if (!find_transcode_slice(a.slices, a.prefix, a.n_slices, a.total_tiles, blockIdx.x * 256u + threadIdx.x, v)) return;
    uint32_t px[16];
    load_tile(a.tiles + (size_t)(v.first_block + v.local) * 4, px);
    const uint32_t unit = unit_bytes(FMT);
    const uint32_t bx = v.local % v.g.nbx, by = v.local / v.g.nbx;
    BU_UNROLL
    for (uint32_t y = 0; y < 4; y++) {
        const uint32_t row = by * 4u + y;
        if (row >= v.g.height) break;
        uint32_t p[4];
        BU_UNROLL
        for (uint32_t x = 0; x < 4; x++) p[x] = pack_pixel(px[y * 4 + x], FMT);
        store_tile_row(unit, a.out + v.out_offset + ((size_t)row * v.g.width + bx * 4u) * unit, bx, v.g.width, p);
    }
}

uint32_t dds_pack_unit_bytes(uint32_t format) { return unit_bytes(format); }
bool dds_pack_is_block_format(uint32_t format) { return is_block_format(format); }

template <uint32_t FMT>
static hipError_t launch_blocks(hipStream_t st, const void* d_tiles, uint32_t n_tiles, void* d_out) {
    hipLaunchKernelGGL((k_dds_pack_blocks<FMT>), dim3((n_tiles + 255) / 256), dim3(256), 0, st, (const uint4*)d_tiles, d_out, n_tiles);
    return hipGetLastError();
}

hipError_t launch_dds_pack_blocks(hipStream_t st, const void* d_tiles, uint32_t n_tiles, uint32_t format, void* d_out) {
    if (!is_block_format(format)) return hipErrorInvalidValue;
    if (!n_tiles) return hipSuccess;
    switch (format) {
    case FMT_BC1: return launch_blocks<FMT_BC1>(st, d_tiles, n_tiles, d_out);
    case FMT_BC2: return launch_blocks<FMT_BC2>(st, d_tiles, n_tiles, d_out);
    case FMT_BC3: return launch_blocks<FMT_BC3>(st, d_tiles, n_tiles, d_out);
    case FMT_BC4: return launch_blocks<FMT_BC4>(st, d_tiles, n_tiles, d_out);
    default: return launch_blocks<FMT_BC5>(st, d_tiles, n_tiles, d_out);
    }
}

template <uint32_t FMT>
static hipError_t launch_pixels(hipStream_t st, const dds_pixels_args& a) {
    hipLaunchKernelGGL((k_dds_pack_pixels<FMT>), dim3((a.total_tiles + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_dds_pack_pixels(hipStream_t st, const void* d_tiles, const bu_hip_transcode_slice* d_slices, const uint32_t* d_prefix, uint32_t n_slices,
                                  uint32_t total_tiles, uint32_t format, void* d_out) {
    if (!is_pixel_format(format)) return hipErrorInvalidValue;
    if (!n_slices || !total_tiles) return hipSuccess;
    const dds_pixels_args a = { (const uint4*)d_tiles, (uint8_t*)d_out, d_slices, d_prefix, n_slices, total_tiles };
    switch (format) {
    case FMT_A8R8G8B8: return launch_pixels<FMT_A8R8G8B8>(st, a);
    case FMT_A8B8G8R8: return launch_pixels<FMT_A8B8G8R8>(st, a);
    case FMT_R8: return launch_pixels<FMT_R8>(st, a);
    case FMT_R8G8: return launch_pixels<FMT_R8G8>(st, a);
    case FMT_R5G6B5: return launch_pixels<FMT_R5G6B5>(st, a);
    case FMT_A1R5G5B5: return launch_pixels<FMT_A1R5G5B5>(st, a);
    default: return launch_pixels<FMT_A4R4G4B4>(st, a);
    }
}

} // namespace bu
