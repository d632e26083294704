// ssim_kernels.hip -- compute_ssim (encoder/basisu_ssim.cpp) for the three calls of `basisu -compare_ssim` over two resident RGBA8 rasters. The arithmetic is ssim.h's;
// this file only decides which lane does which piece.
//
// The map: one lane per pixel, a workgroup per 16x16 tile. The workgroup first stages its tile and the 5-pixel halo of both rasters in LDS (26x26 samples each, one
// u32 per pixel: the RGBA bytes, or the two lumas for the luma launch), coordinates clamped to the region and every raster read with its own pitch. Then each lane
// walks the 121 taps in the reference's order with 5 x C accumulators in registers (C = 4: the RGBA call; C = 2: channel 0 of the 709 call and of the 601 call side by
// side, the three redundant channels of each luma call are never computed). The weights are a kernel argument: uniform, read through the scalar cache. A tile row is 48
// words apart in LDS, so the two rows a 32-lane half reads fall on disjoint banks.
//
// The mean is the reference's serial running float sum per plane, evaluated with fsum_scan.h: (1) one lane per chunk of kSsimChunk addends adds them in double;
// (2) one workgroup per plane turns the chunk sums into exclusive prefixes -- an approximation of the running state at every chunk start; (3) one lane per chunk builds
// the chunk's stretch for the binade that guess lies in and for the one above; (4) one lane per plane walks the chunks in order, applies a stretch where it is valid
// for the real state and adds the chunk's addends one by one where it is not (a zero, negative-crossing or binade-crossing state, a bad guess). (4) is exact whatever
// (1)-(3) guessed, so the mean has the serial sum's bits.
//
// Bounds: the staging reads pixel (clamp(x, 0, w - 1), clamp(y, 0, h - 1)) with w <= wa, wb and h <= ha, hb -- inside both rasters for any pitch >= width -- and writes
// LDS at row * 48 + column, row and column < 26. A lane writes plane[y * w + x] only for x < w, y < h. The chunk kernels touch chunk c < chunks of plane p < 6 and the
// addends c * kSsimChunk .. min(+kSsimChunk, n) - 1 of it.
#include "ssim_kernels.h"
#include "image_metrics_kernels.h"
#include "launch_dispatch.h"
#include <algorithm>

namespace bu {

static constexpr int kSpan = (int)kSsimTile + 2 * SSIM_RADIUS;   // 26
static constexpr int kRow = 48;                                  // words between tile rows in LDS: = 16 mod 32
static constexpr uint32_t kMapThreads = kSsimTile * kSsimTile;

template <int C>
__global__ __launch_bounds__(kMapThreads) void ssim_map_kernel(const uint32_t* __restrict__ a, uint32_t pitch_a, const uint32_t* __restrict__ b, uint32_t pitch_b, uint32_t w,
                                                              uint32_t h, const ssim_weights k, float* __restrict__ planes, uint32_t plane_stride) {
    __shared__ uint32_t ta[kSpan * kRow], tb[kSpan * kRow];
    const uint32_t x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kSpan * kSpan); i += kMapThreads) {
        const uint32_t ty = i / kSpan, tx = i - ty * kSpan;
        const int gx = min(max((int)(x0 + tx) - SSIM_RADIUS, 0), (int)w - 1), gy = min(max((int)(y0 + ty) - SSIM_RADIUS, 0), (int)h - 1);
        ta[ty * kRow + tx] = ssim_sample<C>(a[(size_t)gy * pitch_a + gx]);
        tb[ty * kRow + tx] = ssim_sample<C>(b[(size_t)gy * pitch_b + gx]);
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % kSsimTile, ly = threadIdx.x / kSsimTile, x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const uint32_t* pa = ta + (ly + SSIM_RADIUS) * kRow + lx + SSIM_RADIUS;
    const uint32_t* pb = tb + (ly + SSIM_RADIUS) * kRow + lx + SSIM_RADIUS;
    float out[C];
    ssim_pixel<C>([&](int xd, int yd, uint32_t& sa, uint32_t& sb) { sa = pa[yd * kRow + xd]; sb = pb[yd * kRow + xd]; }, k, out);
#pragma unroll
    for (int c = 0; c < C; c++) planes[(size_t)c * plane_stride + (size_t)y * w + x] = out[c];
}

// (1) csum[plane * chunks + chunk] = the chunk's addends added in double
__global__ __launch_bounds__(256) void ssim_chunk_sum_kernel(const float* __restrict__ planes, uint32_t n, uint32_t chunks, double* __restrict__ csum) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= SSIM_PLANES * chunks) return;
    const uint32_t p = id / chunks, c = id - p * chunks, i0 = c * kSsimChunk, len = min((uint32_t)kSsimChunk, n - i0);
    const float* v = planes + (size_t)p * n + i0;
    double t = 0.0;
    for (uint32_t i = 0; i < len; i++) t += (double)v[i];
    csum[id] = t;
}

// (2) one workgroup per plane: csum -> its exclusive prefix, in place
__global__ __launch_bounds__(256) void ssim_prefix_kernel(double* __restrict__ csum, uint32_t chunks) {
    __shared__ double total[256];
    double* cs = csum + (size_t)blockIdx.x * chunks;
    const uint32_t per = (chunks + 255u) / 256u, first = min(threadIdx.x * per, chunks), last = min(first + per, chunks);
    double s = 0.0;
    for (uint32_t i = first; i < last; i++) s += cs[i];
    total[threadIdx.x] = s;
    __syncthreads();
    double base = 0.0;
    for (uint32_t j = 0; j < threadIdx.x; j++) base += total[j];
    for (uint32_t i = first; i < last; i++) {
        const double v = cs[i];
        cs[i] = base;
        base += v;
    }
}

// (3) the chunk's two stretches for the guessed binade
__global__ __launch_bounds__(256) void ssim_stretch_kernel(const float* __restrict__ planes, uint32_t n, uint32_t chunks, const double* __restrict__ prefix,
                                                          ssim_chunk* __restrict__ summary) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= SSIM_PLANES * chunks) return;
    const uint32_t p = id / chunks, c = id - p * chunks, i0 = c * kSsimChunk, len = min((uint32_t)kSsimChunk, n - i0);
    summary[id] = ssim_chunk_build(planes + (size_t)p * n + i0, len, prefix[id]);
}

// (4) one workgroup per plane: 64 summaries at a time into LDS, lane 0 walks them in order
__global__ __launch_bounds__(64) void ssim_walk_kernel(const float* __restrict__ planes, uint32_t n, uint32_t chunks, const ssim_chunk* __restrict__ summary,
                                                      ssim_device_result* __restrict__ out) {
    __shared__ ssim_chunk batch[64];
    const uint32_t p = blockIdx.x;
    const float* v = planes + (size_t)p * n;
    uint32_t state = 0, walked = 0;   // the sum starts at +0
    for (uint32_t base = 0; base < chunks; base += 64u) {   // uniform: the barriers are reached by all 64 lanes
        if (base + threadIdx.x < chunks) batch[threadIdx.x] = summary[(size_t)p * chunks + base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t count = min(64u, chunks - base);
            for (uint32_t j = 0; j < count; j++) {
                const uint32_t i0 = (base + j) * kSsimChunk;
                state = ssim_chunk_walk(state, batch[j], v + i0, min((uint32_t)kSsimChunk, n - i0), &walked);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->mean[p] = ssim_div(ssim_float(state), static_cast<float>(n));
        out->walked[p] = walked;
    }
}

hipError_t launch_ssim(hipStream_t st, const uint32_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint32_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                       const ssim_weights& weights, void* d_work, bool reduce) {
    const uint32_t w = std::min(wa, wb), h = std::min(ha, hb);
    if (!w || !h || w > kImageMetricsMaxDim || h > kImageMetricsMaxDim || (uint64_t)w * h > kSsimMaxPixels || pitch_a < wa || pitch_b < wb || !d_work) return hipErrorInvalidValue;
    const uint32_t n = w * h, chunks = ssim_chunks(n);
    char* work = static_cast<char*>(d_work);
    float* planes = reinterpret_cast<float*>(work);
    const dim3 grid((w + kSsimTile - 1) / kSsimTile, (h + kSsimTile - 1) / kSsimTile);
    hipLaunchKernelGGL(ssim_map_kernel<4>, grid, dim3(kMapThreads), 0, st, a, pitch_a, b, pitch_b, w, h, weights, planes, n);
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_map_kernel<2>, grid, dim3(kMapThreads), 0, st, a, pitch_a, b, pitch_b, w, h, weights, planes + (size_t)SSIM_PLANE_709 * n, n);
    BU_LAUNCH_CHECK();
    if (!reduce) return hipSuccess;
    double* csum = reinterpret_cast<double*>(work + ssim_prefix_offset(n));
    ssim_chunk* summary = reinterpret_cast<ssim_chunk*>(work + ssim_summary_offset(n));
    const uint32_t per_chunk_grid = (SSIM_PLANES * chunks + 255u) / 256u;
    hipLaunchKernelGGL(ssim_chunk_sum_kernel, dim3(per_chunk_grid), dim3(256), 0, st, planes, n, chunks, csum);
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_prefix_kernel, dim3(SSIM_PLANES), dim3(256), 0, st, csum, chunks);
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_stretch_kernel, dim3(per_chunk_grid), dim3(256), 0, st, planes, n, chunks, csum, summary);
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_walk_kernel, dim3(SSIM_PLANES), dim3(64), 0, st, planes, n, chunks, summary, reinterpret_cast<ssim_device_result*>(work + ssim_result_offset(n)));
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace bu
