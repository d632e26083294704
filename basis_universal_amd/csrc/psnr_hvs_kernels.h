// psnr_hvs_kernels.h -- launchers of psnr_hvs_kernels.hip: the per-block sums of psnr_hvs_compute_chan (psnr_hvs.h) for all six modes over two resident RGBA8 rasters.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bu {

// what the kernels leave on the device: per mode (psnr_hvs.h's HVS_Y_8BIT .. HVS_A), the sum over all blocks of the block's HVS and HVS-M double
struct psnr_hvs_device_sums { double sum_hvs[6], sum_hvsm[6]; };

enum : uint32_t { kPsnrHvsMaxGrid = 2048 };   // workgroups of the block kernel; each leaves 12 partial sums

inline uint32_t psnr_hvs_blocks(uint32_t width, uint32_t height) { return ((width + 7) / 8) * ((height + 7) / 8); }
// bytes of the partial sums the block kernel needs at d_partials (8-byte aligned), whatever the region
inline size_t psnr_hvs_partial_bytes() { return (size_t)kPsnrHvsMaxGrid * 12 * sizeof(double); }

// Compares the 8x8 blocks of the region min(wa, wb) x min(ha, hb); a block's pixel coordinates are clamped to each image's own last column and row. Pixels of 4 bytes,
// pitches in pixels (>= the width), both pointers 4-byte aligned, widths and heights of the region <= kImageMetricsMaxDim. *d_out is cleared on the stream first; an
// empty region launches nothing else. d_per_block (may be null): [blocks][2] doubles, the HVS and HVS-M sum of every block of mode per_block_mode, blocks in raster
// order. Two launches: the blocks, then a fixed tree over the workgroups' partial sums -- the same bits on every run.
hipError_t launch_psnr_hvs(hipStream_t st, const uint32_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint32_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                           double* d_partials, psnr_hvs_device_sums* d_out, double* d_per_block, uint32_t per_block_mode);

}  // namespace bu
