// etc1s_misc_kernels.hip -- the small one-thread-per-item kernels around the fits: a7 the endpoint training vectors, the sub-block errors, the backend's block
// errors, and the tiling of an RGBA raster into 4x4 blocks. Design rules of the ETC1S kernels: etc1s_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "etc1s_device.h"
#include "etc1s_kernels.h"
#include "launch_dispatch.h"
#include "tile_raster.h"

namespace bu {

// -------------------------------------------------------------------------------------------------------------------
// a7: init_endpoint_training_vectors (frontend.cpp:825-866)
// -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_endpoint_training_vectors(const uint64_t* __restrict__ etc_blocks, uint32_t n_blocks, float* __restrict__ out6) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    uint32_t r5, g5, b5, inten;
    unpack_etc1s_header(etc_blocks[i], r5, g5, b5, inten);
    const int br = scale5((int)r5), bg = scale5((int)g5), bb = scale5((int)b5), d = k_inten_b[inten];
    float* o = out6 + (size_t)i * 6;
    const float k = 1.0f / 255.0f; // the reference multiplies by the rounded reciprocal (frontend.cpp:846-851)
    o[0] = (float)clamp255(br - d) * k; o[1] = (float)clamp255(bg - d) * k; o[2] = (float)clamp255(bb - d) * k;
    o[3] = (float)clamp255(br + d) * k; o[4] = (float)clamp255(bg + d) * k; o[5] = (float)clamp255(bb + d) * k;
}

hipError_t launch_endpoint_training_vectors(hipStream_t st, const void* d_etc_blocks, uint32_t n_blocks, float* d_out6) {
    if (!n_blocks) return hipSuccess;
    hipLaunchKernelGGL(k_endpoint_training_vectors, dim3((n_blocks + 255) / 256), dim3(256), 0, st, static_cast<const uint64_t*>(d_etc_blocks), n_blocks, d_out6);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

// compute_endpoint_subblock_error_vec (frontend.cpp:1006-1091): error of every sub-block (training vector) under its cluster's endpoints
template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_subblock_errors(const uint32_t* __restrict__ pixel_words, uint32_t n_blocks, const uint32_t* __restrict__ block_cluster,
                                                         const uint32_t* __restrict__ cluster_params, uint64_t* __restrict__ out) {
    const uint32_t tv = blockIdx.x * 256u + threadIdx.x;
    if (tv >= n_blocks * 2u) return;
    const uint32_t prm = cluster_params[block_cluster[tv >> 1]];
    cvec bc[4];
    // NOT scale5(): the reference passes the 5-bit colour with scaled = true here (frontend.cpp:1043), so the sub-block errors that
    // rank candidates for new clusters are measured against the unscaled values; reproduced as is
    block_cvecs<PERCEPTUAL>(bc, (int)(prm & 255u), (int)((prm >> 8) & 255u), (int)((prm >> 16) & 255u), (int)(prm >> 24));
    uint64_t tot = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) tot += min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(pixel_words[(size_t)tv * 8 + k]), bc);
    out[tv] = tot;
}

hipError_t launch_subblock_errors(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                                  bool perceptual, uint64_t* d_out) {
    if (!n_blocks) return hipSuccess;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_subblock_errors<decltype(p)::value>, dim3((n_blocks * 2 + 255) / 256), dim3(256), 0, st, static_cast<const uint32_t*>(d_pixel_blocks), n_blocks,
                           d_block_cluster, reinterpret_cast<const uint32_t*>(d_cluster_params), d_out);
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

// The stateless part of basisu_backend::create_encoder_blocks (backend.cpp:406-617): for every block of a slice the error of the block as the
// frontend left it (cur_err of :507 and :841) and -- where no causal neighbour already shares its endpoints -- its error under the endpoints of its left, upper and
// upper-left neighbours with its own selectors (what :520-574 evaluates when those neighbours keep their endpoints). One thread per block, tiles and blocks resident;
// the decisions that chain from block to block stay on the host. ~0u: not applicable (edge, shared endpoints, zero error, index out of range).
template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_backend_block_errors(const uint4* __restrict__ pixel_blocks, const uint64_t* __restrict__ etc_blocks, const uint32_t* __restrict__ block_cluster,
                                                              const uint32_t* __restrict__ cluster_params, uint32_t first, uint32_t nbx, uint32_t nby, uint32_t n_clusters,
                                                              int with_neighbours, uint32_t* __restrict__ own, uint32_t* __restrict__ neighbour) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nbx * nby) return;
    const uint32_t b = first + i, bx = i % nbx, by = i / nbx;
    uint32_t px[16];
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint4 v = pixel_blocks[(size_t)b * 4 + k]; px[k * 4] = v.x; px[k * 4 + 1] = v.y; px[k * 4 + 2] = v.z; px[k * 4 + 3] = v.w; }
    const uint64_t mem = etc_blocks[b];
    uint32_t r5, g5, b5, inten;
    unpack_etc1s_header(mem, r5, g5, b5, inten);
    const uint32_t lo32 = (uint32_t)bswap64(mem);
    auto error_under = [&](uint32_t cr, uint32_t cg, uint32_t cb, uint32_t table) {
        cvec bc[4];
        block_cvecs<PERCEPTUAL>(bc, scale5((int)cr), scale5((int)cg), scale5((int)cb), (int)table);
        uint32_t e = 0;
#pragma unroll
        for (uint32_t y = 0; y < 4; y++)
#pragma unroll
            for (uint32_t x = 0; x < 4; x++) e += cdist<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(px[y * 4 + x]), select_cvec(bc, selector_from_bits(lo32, x, y)));
        return e;
    };
    const uint32_t mine_err = error_under(r5, g5, b5, inten);
    own[b] = mine_err;
    if (!with_neighbours) return;
    const uint32_t mine = block_cluster[b];
    const int dx[3] = { -1, 0, -1 }, dy[3] = { 0, -1, -1 };   // g_endpoint_preds (backend.cpp:120-128)
    uint32_t nb[3];
    bool any_equal = false;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const int x = (int)bx + dx[p], y = (int)by + dy[p];
        nb[p] = (x >= 0 && y >= 0) ? block_cluster[first + (uint32_t)x + (uint32_t)y * nbx] : ~0u;
        any_equal = any_equal || nb[p] == mine;
    }
#pragma unroll
    for (int p = 0; p < 3; p++) {
        uint32_t e = ~0u;
        if (mine_err && !any_equal && nb[p] != ~0u && nb[p] < n_clusters) {
            const uint32_t prm = cluster_params[nb[p]];
            e = error_under(prm & 255u, (prm >> 8) & 255u, (prm >> 16) & 255u, prm >> 24);
        }
        neighbour[(size_t)b * 3 + p] = e;
    }
}

hipError_t launch_backend_block_errors(hipStream_t st, const void* d_pixel_blocks, const void* d_etc_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                                       uint32_t first_block, uint32_t nbx, uint32_t nby, uint32_t n_clusters, bool perceptual, bool with_neighbours, uint32_t* d_own,
                                       uint32_t* d_neighbour) {
    if (!nbx || !nby) return hipSuccess;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_backend_block_errors<decltype(p)::value>, dim3((nbx * nby + 255) / 256), dim3(256), 0, st, static_cast<const uint4*>(d_pixel_blocks),
                           static_cast<const uint64_t*>(d_etc_blocks), d_block_cluster, reinterpret_cast<const uint32_t*>(d_cluster_params), first_block, nbx, nby, n_clusters,
                           with_neighbours ? 1 : 0, d_own, d_neighbour);
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

// -------------------------------------------------------------------------------------------------------------------
// Input side: basis_compressor::extract_source_blocks (comp.cpp:3207-3268) = image::extract_block_clamped
// per 4x4 block. One lane per block row: a 16-byte read of four texels (clamped at the right / bottom edges) and a 16-byte write,
// so an RGBA raster can be uploaded once and tiled where it lives.
// -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_extract_blocks(const uint8_t* __restrict__ rgba, uint32_t width, uint32_t height, uint32_t pitch,
                                                        uint32_t blocks_x, uint32_t n_blocks, uint4* __restrict__ out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t block = t >> 2, row = t & 3u;
    if (block >= n_blocks) return;
    const uint32_t bx = block % blocks_x, by = block / blocks_x;
    out[(size_t)block * 4u + row] = load_tile_row_clamped(rgba, pitch, width, height, bx, by * 4u + row);
}

hipError_t launch_extract_blocks(hipStream_t st, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out_blocks) {
    if (!width || !height) return hipSuccess;
    const uint32_t bx = (width + 3) / 4, by = (height + 3) / 4, n = bx * by;
    hipLaunchKernelGGL(k_extract_blocks, dim3((n * 4 + 255) / 256), dim3(256), 0, st, static_cast<const uint8_t*>(d_rgba), width, height, pitch_bytes, bx, n,
                       static_cast<uint4*>(d_out_blocks));
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

// The same for every slice of a call in ONE launch (bu_hip_k_extract_slices): a multi-image call -- array layers, cubemap faces, video frames, each with its levels,
// for ETC1S with alpha a colour and an alpha slice per level -- has hundreds of slices of a few blocks, and a launch pair per slice costs more than the tiling.
// One lane per block row over the tiles of all slices in call order; `prefix` (n_slices + 1 entries, strictly ascending, prefix[n_slices] = total_tiles) says where
// each slice's tiles begin in that order. A wave's lanes are 16 consecutive tiles: find_slice (tile_raster.h) with item = tile, so a lane steps on from the wave's
// first slice at most 15 times, where a wave straddles slices of one block.
// mode 1 / 2 are the ETC1S colour / alpha slices read straight from the RGBA raster (comp.cpp:2883-2903), so no split plane is ever materialised.
__global__ __launch_bounds__(256) void k_extract_slices(const bu_hip_slice_source* __restrict__ slices, const uint32_t* __restrict__ prefix, uint32_t n_slices,
                                                        uint32_t total_tiles, uint4* __restrict__ out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;   // total_tiles <= 2^30 (the launcher's caller refuses more)
    const uint32_t tile = t >> 2, row = t & 3u;
    uint32_t s, local;
    if (!find_slice(prefix, n_slices, total_tiles, tile, s, local)) return;   // every lane of the wave gets here
    const uint4* rec = reinterpret_cast<const uint4*>(slices + s);
    const uint4 r0 = rec[0], r1 = rec[1];                 // { raster lo, hi, width, height } { pitch, mode, first_block lo, hi }
    const uint8_t* rgba = reinterpret_cast<const uint8_t*>((uintptr_t)r0.x | ((uintptr_t)r0.y << 32));
    const uint32_t width = r0.z, height = r0.w, pitch = r1.x, mode = r1.y;
    const uint64_t first_block = (uint64_t)r1.z | ((uint64_t)r1.w << 32);
    const uint32_t blocks_x = (width + 3u) >> 2, bx = local % blocks_x, by = local / blocks_x;
    uint4 v = load_tile_row_clamped(rgba, pitch, width, height, bx, by * 4u + row);
    if (mode == BU_HIP_SLICE_RGB) {
        v.x |= 0xff000000u; v.y |= 0xff000000u; v.z |= 0xff000000u; v.w |= 0xff000000u;
    } else if (mode == BU_HIP_SLICE_ALPHA) {
        v.x = (v.x >> 24) * 0x010101u | 0xff000000u; v.y = (v.y >> 24) * 0x010101u | 0xff000000u;
        v.z = (v.z >> 24) * 0x010101u | 0xff000000u; v.w = (v.w >> 24) * 0x010101u | 0xff000000u;
    }
    out[(size_t)(first_block + local) * 4u + row] = v;
}

hipError_t launch_extract_slices(hipStream_t st, const bu_hip_slice_source* d_slices, const uint32_t* d_prefix, uint32_t n_slices, uint32_t total_tiles, void* d_out_blocks) {
    if (!n_slices || !total_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_extract_slices, dim3((uint32_t)(((uint64_t)total_tiles * 4u + 255u) / 256u)), dim3(256), 0, st, d_slices, d_prefix, n_slices, total_tiles,
                       static_cast<uint4*>(d_out_blocks));
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace bu
