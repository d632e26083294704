// ssim_kernels.h -- launchers of ssim_kernels.hip: the smap planes of compute_ssim (ssim.h) for the RGBA call and both luma calls over two resident RGBA8 rasters, and
// their means as the reference's serial running binary32 sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "ssim_reduce.h"

namespace bu {

enum : uint32_t { kSsimChunk = 256 };            // addends per chunk of the reduction: one stretch pair each (tests and tools read this line)
enum : uint32_t { kSsimTile = 16 };              // a workgroup of the map kernel computes kSsimTile x kSsimTile pixels
enum : uint32_t { kSsimMaxPixels = 1u << 25 };   // the region a context serves: six planes of 128 MiB each at the most

// what the kernels leave on the device: per plane (ssim.h's SSIM_PLANE_*) the mean, and how many of the plane's chunks the walk had to add one by one
struct ssim_device_result { float mean[SSIM_PLANES]; uint32_t walked[SSIM_PLANES]; };

inline uint32_t ssim_chunks(uint32_t pixels) { return (pixels + kSsimChunk - 1) / kSsimChunk; }
// the layout of the work area at d_work (256-byte aligned): the planes [6][pixels] float, the chunk prefixes [6][chunks] double, the chunk summaries [6][chunks], the result
inline size_t ssim_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline size_t ssim_prefix_offset(uint32_t pixels) { return ssim_align((size_t)SSIM_PLANES * pixels * sizeof(float)); }
inline size_t ssim_summary_offset(uint32_t pixels) { return ssim_prefix_offset(pixels) + ssim_align((size_t)SSIM_PLANES * ssim_chunks(pixels) * sizeof(double)); }
inline size_t ssim_result_offset(uint32_t pixels) { return ssim_summary_offset(pixels) + ssim_align((size_t)SSIM_PLANES * ssim_chunks(pixels) * sizeof(ssim_chunk)); }
inline size_t ssim_work_bytes(uint32_t pixels) { return ssim_result_offset(pixels) + ssim_align(sizeof(ssim_device_result)); }

// Compares the region w x h = min(wa, wb) x min(ha, hb), 1 <= w * h <= kSsimMaxPixels, w and h <= kImageMetricsMaxDim; filter coordinates are clamped to the REGION
// (compute_ssim crops both images first). Pixels of 4 bytes, pitches in pixels (>= the width), both pointers 4-byte aligned. Writes the six planes (raster order,
// plane p at ((float*)d_work)[p * w * h ...]) and, with reduce set, the result at d_work + ssim_result_offset(w * h). Two launches for the planes, four for the means.
hipError_t launch_ssim(hipStream_t st, const uint32_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint32_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                       const ssim_weights& weights, void* d_work, bool reduce);

}  // namespace bu
