// texture_unpack_kernels.hip -- gpu_image::unpack (encoder/basisu_gpu_texture.cpp:1218-1266) over resident blocks of every format this package's transcoders write:
// the same shape as block_unpack_kernels.hip -- one lane per TEXEL, 16 lanes per block, 4 blocks per wave, 16 blocks per workgroup, the format a template parameter
// so that each instance carries only its own path (texture_unpack.h) -- kept in a file of its own so that the five instances there keep their code.
// The 16 lanes of a block load its 8 or 16 bytes from one address (one request, broadcast), decode the header redundantly and each extract only what their texel
// needs; for ASTC that is the partition of the texel, the BISE groups that hold that partition's endpoint values and the groups that hold the up to four (dual
// plane: eight) grid weights around it. Nothing is an array indexed by a run-time value. A lane stores one uint32; only width x height pixels (rows cut at `rows`)
// are written. An invalid block gets zeros and is counted with a vector atomic by its first lane; it never stops the others.
// PVRTC1 is an instance of its own: the lane's block lies at its Morton address, and the texel blends the endpoint words of the 2x2 blocks around it (wrapped at
// the edges: nbx and nby are powers of two), four 4-byte loads that the 16 lanes of a block share between nine addresses.
#include <hip/hip_runtime.h>
#include "texture_unpack.h"
#include "texture_unpack_kernels.h"

namespace bu {
using namespace bu_unpack;

template <uint32_t FORMAT>
__global__ __launch_bounds__(256) void unpack_texture_kernel(texture_unpack_args a) {
    const tile_geometry& g = a.g;
    const uint32_t n = g.nbx * g.nby, b = blockIdx.x * 16u + (threadIdx.x >> 4), i = threadIdx.x & 15u;   // n <= 2^28: no overflow
    if (b >= n) return;
    uint64_t lo, hi = 0;
    if (texture_bytes_per_block(FORMAT) == 8u) {
        const uint2 in = ((const uint2*)a.blocks)[b];
        lo = (uint64_t)in.x | ((uint64_t)in.y << 32);
    } else {
        const uint4 in = ((const uint4*)a.blocks)[b];
        lo = (uint64_t)in.x | ((uint64_t)in.y << 32);
        hi = (uint64_t)in.z | ((uint64_t)in.w << 32);
    }
    bool ok;
    const uint32_t px = unpack_texture_texel<FORMAT>(lo, hi, i, &ok);
    if (!ok && i == 0u) atomicAdd(a.invalid, 1u);
    const uint32_t bx = b % g.nbx, by = b / g.nbx, x = bx * 4u + (i & 3u), y = by * 4u + (i >> 2);
    if (x < g.width && y < g.height && y < g.rows) a.out[(size_t)y * g.pitch + x] = px;
}

__global__ __launch_bounds__(256) void unpack_pvrtc1_kernel(texture_unpack_args a) {
    const tile_geometry& g = a.g;
    const uint32_t n = g.nbx * g.nby, b = blockIdx.x * 16u + (threadIdx.x >> 4), i = threadIdx.x & 15u;
    if (b >= n) return;
    const uint32_t bx = b % g.nbx, by = b / g.nbx;
    // the 2x2 blocks around the texel: the block itself and the one before it (x, y < 2) or after it, wrapped; every address is below nbx * nby
    const uint32_t x0 = ((i & 3u) < 2u ? bx + g.nbx - 1u : bx) & (g.nbx - 1u), x1 = (x0 + 1u) & (g.nbx - 1u);
    const uint32_t y0 = ((i >> 2) < 2u ? by + g.nby - 1u : by) & (g.nby - 1u), y1 = (y0 + 1u) & (g.nby - 1u);
    const uint2* blocks = (const uint2*)a.blocks;   // .x the modulation bits, .y the endpoint word
    const uint32_t p = blocks[bu_pvrtc1::morton_address(x0, y0, g.nbx, g.nby)].y, q = blocks[bu_pvrtc1::morton_address(x1, y0, g.nbx, g.nby)].y;
    const uint32_t r = blocks[bu_pvrtc1::morton_address(x0, y1, g.nbx, g.nby)].y, s = blocks[bu_pvrtc1::morton_address(x1, y1, g.nbx, g.nby)].y;
    const uint32_t modulation = blocks[bu_pvrtc1::morton_address(bx, by, g.nbx, g.nby)].x;
    const uint32_t px = unpack_texel_pvrtc1(p, q, r, s, modulation, i);
    const uint32_t x = bx * 4u + (i & 3u), y = by * 4u + (i >> 2);
    if (x < g.width && y < g.height && y < g.rows) a.out[(size_t)y * g.pitch + x] = px;
}

template <uint32_t FORMAT>
static hipError_t launch(hipStream_t st, const texture_unpack_args& a) {
    const uint32_t n = a.g.nbx * a.g.nby;
    hipLaunchKernelGGL((unpack_texture_kernel<FORMAT>), dim3((n + 15u) / 16u), dim3(256), 0, st, a);
    return hipGetLastError();
}

uint32_t texture_unpack_bytes_per_block(uint32_t format) { return texture_bytes_per_block(format); }

hipError_t launch_unpack_texture(hipStream_t st, const texture_unpack_args& a, uint32_t format) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !a.g.nbx || !a.g.nby) return e;
    switch (format) {
    case UF_BC1: return launch<UF_BC1>(st, a);
    case UF_BC3: return launch<UF_BC3>(st, a);
    case UF_BC4: return launch<UF_BC4>(st, a);
    case UF_BC5: return launch<UF_BC5>(st, a);
    case UF_BC7: return launch<UF_BC7>(st, a);
    case UF_ETC1: return launch<UF_ETC1>(st, a);
    case UF_ETC2_RGBA: return launch<UF_ETC2_RGBA>(st, a);
    case UF_EAC_R11: return launch<UF_EAC_R11>(st, a);
    case UF_EAC_RG11: return launch<UF_EAC_RG11>(st, a);
    case UF_ASTC_4x4: return launch<UF_ASTC_4x4>(st, a);
    case UF_PVRTC1_RGB:
    case UF_PVRTC1_RGBA: {
        if ((a.g.nbx & (a.g.nbx - 1u)) || (a.g.nby & (a.g.nby - 1u))) return hipErrorInvalidValue;   // the kernel wraps with masks
        const uint32_t n = a.g.nbx * a.g.nby;
        hipLaunchKernelGGL(unpack_pvrtc1_kernel, dim3((n + 15u) / 16u), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    default: return hipErrorInvalidValue;
    }
}

}  // namespace bu
