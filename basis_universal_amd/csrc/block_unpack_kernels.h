// block_unpack_kernels.h -- launcher of block_unpack_kernels.hip: resident BC1 / BC3 / BC4 / BC5 / BC7 blocks -> an RGBA8 raster (gpu_image::unpack on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tile_raster.h"

namespace bu {

struct block_unpack_args {
    const void* blocks;    // nbx * nby blocks of 8 (BC1, BC4) or 16 bytes, raster order, aligned to their size
    uint32_t* out;         // RGBA8 raster, 4-byte aligned
    uint32_t* invalid;     // device counter
    tile_geometry g;       // width x height pixels are written (rows cut at `rows`); pitch in pixels
};

uint32_t block_unpack_bytes_per_block(uint32_t format);   // 0 = the format does not unpack here
// one launch; d_invalid is cleared first and afterwards holds how many BC7 blocks had the reserved mode (their texels are zero-filled)
hipError_t launch_unpack_blocks(hipStream_t st, const block_unpack_args& a, uint32_t format);

}  // namespace bu
