// image_metrics_kernels.hip -- the counting half of image_metrics::calc (encoder/basisu_enc.cpp:2155-2226) for all eight lines of `basisu -stats` in one pass over two
// resident RGBA8 rasters: six 256-bin histograms of absolute differences (R, G, B, A, 709 luma, 601 luma) and the per-channel sums of both images. The float half is
// host code (image_metrics.h, im_reduce). Memory bound: 8 bytes read per pixel pair, nothing written but the counts.
//
// Work unit: four consecutive pixels of one row. A lane reads a unit of each image as one 16-byte word when the unit is whole and its address is 16-byte aligned, and
// pixel by pixel otherwise (the ragged end of a row; every unit of a raster whose rows do not start on 16 bytes), so no byte outside width x height is ever read.
//
// Histograms: the differences of a good encode pile into bins 0-8, and in the degenerate cases (a == b) every lane of every wave hits one bin, so one LDS counter per
// bin would take the 64 adds of a wave-instruction one after the other. Each counter is therefore replicated kReplicas = 8 times by lane (lane & 7), replicas in
// consecutive words: the lanes that meet on one bin spread over 8 banks, and at most 4 lanes of a 32-lane group share an address ("Quality stats"). 6 x 256
// x 8 counters are 48 KiB, three workgroups per CU. A workgroup flushes once, replica sums of the bins it touched, with integer global atomics: whatever the order,
// the counts are the same.
//
// Counter widths at 16384 x 16384 (kImageMetricsMaxDim each way) = 2^28 pixels:
//   global bin, 32 bits   : at most one count per pixel and row, 2^28 = 2.7e8.
//   LDS replica, 32 bits  : at most the pixels one workgroup sees, <= 2^28.
//   per-lane channel sum, 32 bits: a lane takes ceil(units / (grid * 256)) units; units <= 2^26 and grid = min(ceil(units / 256), kMaxGrid = 768), so at most 342 units
//       = 1,368 pixels x 255 = 348,840; a workgroup's sum (x 256) is 8.9e7, still 32 bits.
//   global channel sum, 64 bits: 2^28 x 255 = 6.9e10.
#include "image_metrics_kernels.h"
#include "image_metrics.h"
#include "launch_dispatch.h"
#include <algorithm>

namespace bu {

static constexpr uint32_t kReplicas = 8, kMaxGrid = 768;   // 768 = three resident workgroups (48 KiB of LDS each) on each of 256 CUs

static_assert(sizeof(image_metrics_device_counts) == IM_ROWS * IM_BINS * 4 + 64, "hist, sum_a, sum_b without padding");

__device__ __forceinline__ void count_pixel(uint32_t* hist, uint32_t rep, uint32_t pa, uint32_t pb, uint32_t sa[4], uint32_t sb[4]) {
    uint32_t bins[IM_ROWS];
    im_pixel_bins(pa, pb, bins);
#pragma unroll
    for (uint32_t r = 0; r < IM_ROWS; r++) atomicAdd(&hist[(r * IM_BINS + bins[r]) * kReplicas + rep], 1u);
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        sa[c] += (pa >> (8 * c)) & 255u;
        sb[c] += (pb >> (8 * c)) & 255u;
    }
}

// n <= 4 pixels from p into v; the 16-byte read only where it is whole and aligned
__device__ __forceinline__ void load_unit(const uint32_t* p, uint32_t n, uint32_t v[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = k < n ? p[k] : 0u;
    }
}

__global__ __launch_bounds__(256) void image_metrics_kernel(const uint32_t* __restrict__ a, uint32_t pitch_a, const uint32_t* __restrict__ b, uint32_t pitch_b, uint32_t width,
                                                            uint32_t units_per_row, uint32_t units, image_metrics_device_counts* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[IM_ROWS * IM_BINS * kReplicas];
    __shared__ uint32_t sums[8];
    for (uint32_t i = threadIdx.x; i < IM_ROWS * IM_BINS * kReplicas; i += 256u) hist[i] = 0;
    if (threadIdx.x < 8) sums[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t rep = threadIdx.x & (kReplicas - 1);
    uint32_t sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const uint32_t y = u / units_per_row, x0 = (u - y * units_per_row) * 4u;
        const uint32_t n = min(4u, width - x0);
        uint32_t va[4], vb[4];
        load_unit(a + ((size_t)y * pitch_a + x0), n, va);
        load_unit(b + ((size_t)y * pitch_b + x0), n, vb);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (k < n) count_pixel(hist, rep, va[k], vb[k], sa, sb);
    }
    // channel sums: wave (64 lanes x 348,840 fits 32 bits) -> workgroup -> one 64-bit atomic per sum
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            sa[c] += __shfl_xor(sa[c], ofs);
            sb[c] += __shfl_xor(sb[c], ofs);
        }
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) {
            atomicAdd(&sums[c], sa[c]);
            atomicAdd(&sums[4 + c], sb[c]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) atomicAdd(&out->sum_a[threadIdx.x], (unsigned long long)sums[threadIdx.x]);
    else if (threadIdx.x < 8) atomicAdd(&out->sum_b[threadIdx.x - 4], (unsigned long long)sums[threadIdx.x]);
    uint32_t* out_hist = &out->hist[0][0];
    for (uint32_t i = threadIdx.x; i < IM_ROWS * IM_BINS; i += 256u) {
        const uint4 lo = *reinterpret_cast<const uint4*>(&hist[i * kReplicas]), hi = *reinterpret_cast<const uint4*>(&hist[i * kReplicas + 4]);
        const uint32_t v = lo.x + lo.y + lo.z + lo.w + hi.x + hi.y + hi.z + hi.w;
        if (v) atomicAdd(&out_hist[i], v);
    }
}

hipError_t launch_image_metrics(hipStream_t st, const uint32_t* a, uint32_t pitch_a, const uint32_t* b, uint32_t pitch_b, uint32_t width, uint32_t height,
                                image_metrics_device_counts* d_out) {
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(image_metrics_device_counts), st);
    if (e != hipSuccess || !width || !height) return e;
    if (width > kImageMetricsMaxDim || height > kImageMetricsMaxDim || pitch_a < width || pitch_b < width) return hipErrorInvalidValue;
    const uint32_t units_per_row = (width + 3) / 4, units = units_per_row * height;
    const uint32_t grid = std::min((units + 255u) / 256u, kMaxGrid);
    hipLaunchKernelGGL(image_metrics_kernel, dim3(grid), dim3(256), 0, st, a, pitch_a, b, pitch_b, width, units_per_row, units, d_out);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace bu
