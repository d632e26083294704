// psnr_hvs_kernels.hip -- psnr_hvs_compute_chan (encoder/basisu_enc.cpp:2343-2465) for all six modes of psnr_hvs_compute_metrics in one pass over two resident RGBA8
// rasters. The arithmetic is psnr_hvs.h's; this file only decides which lane calls which piece.
//
// A workgroup is six waves, one per mode, and walks a contiguous run of 8x8 blocks in raster order. Per block the two 64-pixel tiles are read once (clamped to each
// image's own edge) into LDS; then, in every wave, lane i is sample i, then output i of the horizontal DCT pass, then coefficient i of the vertical pass and of the
// term stage. What cannot be spread over lanes without leaving the reference's rounding are the order-fixed float chains -- per image the mean and the sum of squares
// of the block and of its four quadrants, and the masking energy over coefficients 1..63 -- and the two 64-term double sums: each chain is one lane's (lanes 0-9 the
// variances, 16-17 the energies, 0-1 the double sums). The stages hand over through LDS (2 KiB per wave) with a workgroup barrier between them: six per block.
//
// Sums: lanes 0 and 1 of every wave add their block doubles in block order into a register and store one partial per workgroup; a second launch adds the partials of
// each of the twelve sums in a fixed order (strided serial sums in 256 lanes, then a fixed LDS tree). No floating-point atomics: the same bits on every run. Against
// the reference's one running double over all terms this is another association of the same non-negative doubles ("PSNR-HVS").
//
// Bounds: a lane reads pixel min(8 bx + x, w_img - 1), min(8 by + y, h_img - 1) of its image -- inside the raster for any pitch >= width --, writes LDS at indices
// below 64 of its wave's arrays, and global memory at partials[workgroup * 12 + 0..11] (grid <= kPsnrHvsMaxGrid) and per_block[block * 2 + 0..1] (block < blocks).
#include "psnr_hvs_kernels.h"
#include "psnr_hvs.h"
#include "image_metrics_kernels.h"
#include "launch_dispatch.h"
#include <algorithm>

namespace bu {

static constexpr uint32_t kThreads = 64 * HVS_MODES;

__global__ __launch_bounds__(kThreads) void psnr_hvs_blocks_kernel(const uint32_t* __restrict__ a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint32_t* __restrict__ b,
                                                                  uint32_t wb, uint32_t hb, uint32_t pitch_b, uint32_t blocks_x, uint32_t blocks, uint32_t chunk,
                                                                  double* __restrict__ partials, double* __restrict__ per_block, uint32_t per_block_mode) {
    __shared__ uint32_t pix[2][64];
    __shared__ float blk[HVS_MODES][2][64], work[HVS_MODES][2][64], dct[HVS_MODES][2][64], terms[HVS_MODES][2][64];
    __shared__ float chain[HVS_MODES][2][8];   // per image: the five variances, the masking energy
    const uint32_t mode = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t first = blockIdx.x * chunk, last = min(first + chunk, blocks);   // the same for every thread of the workgroup: the barriers below are uniform
    double acc = 0.0;
    for (uint32_t bi = first; bi < last; bi++) {
        if (threadIdx.x < 128) {
            const uint32_t by = bi / blocks_x, bx = bi - by * blocks_x, x = bx * 8 + (lane & 7), y = by * 8 + (lane >> 3);
            pix[mode][lane] = mode ? b[(size_t)min(y, hb - 1) * pitch_b + min(x, wb - 1)] : a[(size_t)min(y, ha - 1) * pitch_a + min(x, wa - 1)];
        }
        __syncthreads();
        blk[mode][0][lane] = hvs_sample(mode, pix[0][lane]);
        blk[mode][1][lane] = hvs_sample(mode, pix[1][lane]);
        __syncthreads();
        work[mode][0][lane] = hvs_dct_horizontal(blk[mode][0], lane >> 3, lane & 7);
        work[mode][1][lane] = hvs_dct_horizontal(blk[mode][1], lane >> 3, lane & 7);
        __syncthreads();
        const float da = hvs_dct_vertical(work[mode][0], lane >> 3, lane & 7), db = hvs_dct_vertical(work[mode][1], lane >> 3, lane & 7);
        dct[mode][0][lane] = da;
        dct[mode][1][lane] = db;
        __syncthreads();
        if (lane < 10) chain[mode][lane / 5][lane % 5] = hvs_variance_k(blk[mode][lane / 5], lane % 5);
        else if (lane == 16 || lane == 17) chain[mode][lane - 16][5] = hvs_mask_energy(dct[mode][lane - 16]);
        __syncthreads();
        const float sa = hvs_mask_strength(chain[mode][0][5], chain[mode][0]), sb = hvs_mask_strength(chain[mode][1][5], chain[mode][1]);
        float th, tm;
        hvs_terms(da, db, lane, sb > sa ? sb : sa, &th, &tm);
        terms[mode][0][lane] = th;
        terms[mode][1][lane] = tm;
        __syncthreads();
        if (lane < 2) {
            const double s = hvs_sum_terms(terms[mode][lane]);
            acc += s;
            if (per_block && mode == per_block_mode) per_block[(size_t)bi * 2 + lane] = s;
        }
    }
    if (lane < 2) partials[((size_t)blockIdx.x * HVS_MODES + mode) * 2 + lane] = acc;
}

// one workgroup per sum j = mode * 2 + (0 = HVS, 1 = HVS-M): partials [n][12] -> out
__global__ __launch_bounds__(256) void psnr_hvs_sum_kernel(const double* __restrict__ partials, uint32_t n, psnr_hvs_device_sums* __restrict__ out) {
    __shared__ double tree[256];
    const uint32_t j = blockIdx.x;
    double s = 0.0;
    for (uint32_t p = threadIdx.x; p < n; p += 256u) s += partials[(size_t)p * (HVS_MODES * 2) + j];
    tree[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t ofs = 128; ofs > 0; ofs >>= 1) {
        if (threadIdx.x < ofs) tree[threadIdx.x] += tree[threadIdx.x + ofs];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j & 1) out->sum_hvsm[j >> 1] = tree[0];
        else out->sum_hvs[j >> 1] = tree[0];
    }
}

hipError_t launch_psnr_hvs(hipStream_t st, const uint32_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint32_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b,
                           double* d_partials, psnr_hvs_device_sums* d_out, double* d_per_block, uint32_t per_block_mode) {
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(psnr_hvs_device_sums), st);
    const uint32_t w = std::min(wa, wb), h = std::min(ha, hb);
    if (e != hipSuccess || !w || !h) return e;
    if (w > kImageMetricsMaxDim || h > kImageMetricsMaxDim || pitch_a < wa || pitch_b < wb || per_block_mode >= HVS_MODES) return hipErrorInvalidValue;
    const uint32_t blocks_x = (w + 7) / 8, blocks = psnr_hvs_blocks(w, h);
    const uint32_t chunk = (blocks + kPsnrHvsMaxGrid - 1) / kPsnrHvsMaxGrid, grid = (blocks + chunk - 1) / chunk;
    hipLaunchKernelGGL(psnr_hvs_blocks_kernel, dim3(grid), dim3(kThreads), 0, st, a, wa, ha, pitch_a, b, wb, hb, pitch_b, blocks_x, blocks, chunk, d_partials, d_per_block,
                       per_block_mode);
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(psnr_hvs_sum_kernel, dim3(HVS_MODES * 2), dim3(256), 0, st, d_partials, grid, d_out);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace bu
