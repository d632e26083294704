// image_metrics_kernels.h -- launcher of image_metrics_kernels.hip: the counting half of image_metrics::calc (image_metrics.h) over two resident RGBA8 rasters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bu {

// what the kernel leaves on the device; the host copy is bu_image_metrics_counts (include/basisu_hip.h) from `hist` on
struct image_metrics_device_counts {
    uint32_t hist[6][256];            // rows: image_metrics.h's IM_R .. IM_LUMA_601
    unsigned long long sum_a[4], sum_b[4];
};

enum : uint32_t { kImageMetricsMaxDim = 16384 };   // the compressor's limit (BASISU_MAX_SUPPORTED_TEXTURE_DIMENSION); the counter widths are argued for it

// Compares a[y * pitch_a + x] with b[y * pitch_b + x] (pixels of 4 bytes; both pointers 4-byte aligned) for x < width, y < height. *d_out is cleared on the stream
// first; an empty region launches nothing else. width, height <= kImageMetricsMaxDim.
hipError_t launch_image_metrics(hipStream_t st, const uint32_t* a, uint32_t pitch_a, const uint32_t* b, uint32_t pitch_b, uint32_t width, uint32_t height,
                                image_metrics_device_counts* d_out);

}  // namespace bu
