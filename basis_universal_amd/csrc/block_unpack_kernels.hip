// block_unpack_kernels.hip -- gpu_image::unpack (encoder/basisu_gpu_texture.cpp:1218-1266) over resident BC1 / BC3 / BC4 / BC5 / BC7 blocks: one lane per TEXEL,
// 16 lanes per block, 4 blocks per wave, 16 blocks per workgroup, the format a template parameter so that each instance carries only its own path (block_unpack.h).
// The 16 lanes of a block load its 8 or 16 bytes from one address (one request, broadcast), decode the header redundantly and each extract only their own index:
// nothing is an array indexed by a run-time value, so an instance has no scratch, and BC7's eight modes can diverge only between the four blocks of a wave. A lane
// stores one uint32; a block's row is 16 contiguous bytes, four x-adjacent blocks give 64. Only width x height pixels (rows cut at `rows`) are written: ragged right
// and bottom blocks are clipped, a padded pitch and rows past `rows` stay untouched. A BC7 block of the reserved mode (byte 0 == 0) gets zeros and is counted with a
// vector atomic by its first lane; it never stops the others.
#include <hip/hip_runtime.h>
#include "block_unpack.h"
#include "block_unpack_kernels.h"

namespace bu {
using namespace bu_unpack;

template <uint32_t FORMAT>
__global__ __launch_bounds__(256) void unpack_blocks_kernel(block_unpack_args a) {
    const tile_geometry& g = a.g;
    const uint32_t n = g.nbx * g.nby, b = blockIdx.x * 16u + (threadIdx.x >> 4), i = threadIdx.x & 15u;   // n <= 2^28: no overflow
    if (b >= n) return;
    uint64_t lo, hi = 0;
    if (unpack_bytes_per_block(FORMAT) == 8u) {
        const uint2 in = ((const uint2*)a.blocks)[b];
        lo = (uint64_t)in.x | ((uint64_t)in.y << 32);
    } else {
        const uint4 in = ((const uint4*)a.blocks)[b];
        lo = (uint64_t)in.x | ((uint64_t)in.y << 32);
        hi = (uint64_t)in.z | ((uint64_t)in.w << 32);
    }
    bool ok;
    const uint32_t px = unpack_texel<FORMAT>(lo, hi, i, &ok);
    if (FORMAT == UF_BC7 && !ok && i == 0u) atomicAdd(a.invalid, 1u);
    const uint32_t bx = b % g.nbx, by = b / g.nbx, x = bx * 4u + (i & 3u), y = by * 4u + (i >> 2);
    if (x < g.width && y < g.height && y < g.rows) a.out[(size_t)y * g.pitch + x] = px;
}

template <uint32_t FORMAT>
static hipError_t launch(hipStream_t st, const block_unpack_args& a) {
    const uint32_t n = a.g.nbx * a.g.nby;
    hipLaunchKernelGGL((unpack_blocks_kernel<FORMAT>), dim3((n + 15u) / 16u), dim3(256), 0, st, a);
    return hipGetLastError();
}

uint32_t block_unpack_bytes_per_block(uint32_t format) { return unpack_bytes_per_block(format); }

hipError_t launch_unpack_blocks(hipStream_t st, const block_unpack_args& a, uint32_t format) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !a.g.nbx || !a.g.nby) return e;
    switch (format) {
    case UF_BC1: return launch<UF_BC1>(st, a);
    case UF_BC3: return launch<UF_BC3>(st, a);
    case UF_BC4: return launch<UF_BC4>(st, a);
    case UF_BC5: return launch<UF_BC5>(st, a);
    case UF_BC7: return launch<UF_BC7>(st, a);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace bu
