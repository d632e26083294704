// texture_unpack_kernels.h -- launcher of texture_unpack_kernels.hip: resident blocks of any format this package's transcoders write -> an RGBA8 raster
// (gpu_image::unpack on the device): the five BC formats, ETC1, ETC2 RGBA, EAC R11 / RG11, ASTC 4x4 (LDR, L8 profile) and PVRTC1 4bpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tile_raster.h"

namespace bu {

struct texture_unpack_args {
    const void* blocks;    // nbx * nby blocks of 8 or 16 bytes, aligned to their size; raster order, PVRTC1 in its own Morton order
    uint32_t* out;         // RGBA8 raster, 4-byte aligned
    uint32_t* invalid;     // device counter
    tile_geometry g;       // width x height pixels are written (rows cut at `rows`); pitch in pixels. PVRTC1: nbx and nby are powers of two
};

uint32_t texture_unpack_bytes_per_block(uint32_t format);   // 0 = the format does not unpack here
// one launch; d_invalid is cleared first and afterwards holds how many blocks were invalid (BC7's reserved mode, an ETC1 / ETC2 colour half whose differential
// base overflows, an ASTC block the LDR decoder refuses); their texels are zero-filled
hipError_t launch_unpack_texture(hipStream_t st, const texture_unpack_args& a, uint32_t format);

}  // namespace bu
