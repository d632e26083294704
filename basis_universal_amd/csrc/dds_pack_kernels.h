// dds_pack_kernels.h -- host-side launch interface of dds_pack_kernels.hip (internal to libbasisu_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/basisu_hip.h"

namespace bu {

// bytes per block (BC1-BC5) or per pixel (the raw formats) of a BU_HIP_DDS_* format; 0 for BC7 and for anything that is no format
uint32_t dds_pack_unit_bytes(uint32_t format);
bool dds_pack_is_block_format(uint32_t format);   // BC1-BC5
// One launch over n_tiles resident tiles (64 B each, RGBA8, rows of four texels), stream-ordered: tile i -> 8 or 16 bytes at d_out + i * unit.
// hipErrorInvalidValue for a format that is not BC1-BC5.
hipError_t launch_dds_pack_blocks(hipStream_t st, const void* d_tiles, uint32_t n_tiles, uint32_t format, void* d_out);
// One launch over the tiles of every slice of a table (find_transcode_slice's, tile_raster.h: device copies of the records with their zero sizes filled in, d_prefix
// [n_slices + 1] strictly ascending): slice s reads its tiles from d_tiles + 64 * first_block and writes width x height pixels in tight rows at d_out + out_offset.
// hipErrorInvalidValue for a format that is not one of the seven raw ones.
hipError_t launch_dds_pack_pixels(hipStream_t st, const void* d_tiles, const bu_hip_transcode_slice* d_slices, const uint32_t* d_prefix, uint32_t n_slices,
                                  uint32_t total_tiles, uint32_t format, void* d_out);

} // namespace bu
