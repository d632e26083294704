// uastc_transcode_kernels.h -- host-side launch interface of uastc_transcode_kernels.hip (internal to libbasisu_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/basisu_hip.h"
#include "tile_raster.h"

namespace bu {

// Bytes the transcode of an nbx x nby grid writes for `target` (a transcoder_texture_format value); RGBA32: the tight width x height raster (0 = the
// padded size). 0 for a target that is not supported.
size_t transcode_output_bytes(uint32_t nbx, uint32_t nby, uint32_t width, uint32_t height, uint32_t target);
// One launch over the grid, stream-ordered. g: the grid, the image's size (<= the grid's) and the RGBA32 raster's row pitch and row count in pixels, no zeros
// left; chan0 / chan1: BC4's channel, BC5's two. *d_invalid (device) receives the number of blocks that did not unpack (zero-filled).
// texture_family: the dispatch of bu_hip_k_transcode_uastc_texture(s) -- also ETC1, ETC2 RGBA, EAC R11 / RG11 (chan0 / chan1 as BC4 / BC5) and the 16-bit rasters
// (pitch and rows as RGBA32). Without it those targets answer hipErrorInvalidValue, as every target outside the first family's seven does.
hipError_t launch_transcode_uastc(hipStream_t st, const void* d_blocks, const tile_geometry& g, uint32_t target, bool high_quality, uint32_t chan0, uint32_t chan1,
                                  void* d_out, uint32_t* d_invalid, bool texture_family = false);
// The same for every slice of a table in ONE launch (bu_hip_k_transcode_uastc_slices): d_slices are device copies of the records with every zero size replaced by what
// it stands for, d_prefix[n_slices + 1] where each slice's blocks begin among the total_blocks of the call (strictly ascending). Slice s reads its blocks from
// d_blocks + 16 * first_block and writes at d_out + out_offset; d_invalid[n_slices] is cleared first and receives the per-slice counts.
hipError_t launch_transcode_uastc_slices(hipStream_t st, const void* d_blocks, const bu_hip_transcode_slice* d_slices, const uint32_t* d_prefix, uint32_t n_slices,
                                         uint32_t total_blocks, uint32_t target, bool high_quality, uint32_t chan0, uint32_t chan1, void* d_out, uint32_t* d_invalid,
                                         bool texture_family = false);
// the texture family's unit: bytes per block of a block target, per pixel of a pixel target (RGBA32 and the 16-bit formats); 0 = not one of its targets
uint32_t uastc_texture_unit_bytes(uint32_t target);
bool uastc_texture_is_pixel_target(uint32_t target);

} // namespace bu
