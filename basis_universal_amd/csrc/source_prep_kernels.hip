// source_prep_kernels.hip -- the source-image options of basis_compressor::read_source_images (renormalise, swizzle, alpha policy, vertical flip: source_prep.h) in
// ONE pass over a resident RGBA8 raster, and the ETC1S alpha split (one read, two writes). Bandwidth kernels: a lane owns four x-adjacent pixels of one row, a wave one
// 1 KiB stretch of a row, a workgroup (64 x 4) four rows; the grid is bounded and strides over the rest. Where a lane's four pixels are whole and both addresses are
// 16-byte aligned it moves one uint4 each way, as the ETC1S transcoder's pixel targets do; a ragged last quad, or a row that starts off a 16-byte line, goes pixel by
// pixel and never past `width`. The four pixels live in named registers (constant indices after unrolling): no scratch.
// The flip is the row the lane READS (height - 1 - y), so writes stay in raster order; in place it would read rows already overwritten, and the C ABI refuses that.
// "Any prepared alpha below 255" is OR-ed per lane over its pixels, then per wave with a ballot, and one lane of a wave that saw one does one vector atomicOr --
// unless a relaxed load shows the bit already set: on an image with alpha everywhere every wave would otherwise queue at one address (measured at 4096^2 with one
// workgroup per 256 x 4 pixels: 65,536 atomics, 0.756 ms against 0.071 ms now). The grid is bounded to 2,048 workgroups (eight waves per SIMD on 256 CUs) for the same
// reason: few waves, each striding over rows.
#include <hip/hip_runtime.h>
#include "launch_dispatch.h"
#include "source_prep_kernels.h"

namespace bu {

enum : uint32_t { SP_BLOCK_X = 64, SP_BLOCK_Y = 4, SP_MAX_GRID_X = 64, SP_MAX_GRID = 2048 };
#define SP_GREY_OPAQUE 0xFF808080u   // what a lane holds for the pixels past the row's end: renormalisation skips it, it is not below 255, and it is never stored

__device__ __forceinline__ void load_quad(const uint8_t* s, uint32_t n, uint32_t (&v)[4]) {
    if (n == 4u && ((uintptr_t)s & 15u) == 0u) {
        const uint4 in = *(const uint4*)s;
        v[0] = in.x; v[1] = in.y; v[2] = in.z; v[3] = in.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) v[k] = k < n ? ((const uint32_t*)s)[k] : SP_GREY_OPAQUE;
    }
}

__device__ __forceinline__ void store_quad(uint8_t* d, uint32_t n, const uint32_t (&v)[4]) {
    if (n == 4u && ((uintptr_t)d & 15u) == 0u) {
        *(uint4*)d = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (k < n) ((uint32_t*)d)[k] = v[k];
    }
}

template <bool RENORM>
__global__ __launch_bounds__(SP_BLOCK_X * SP_BLOCK_Y) void prepare_source_kernel(source_prep_args a) {
    const uint32_t quads = (a.width + 3u) >> 2;   // width <= 16384
    const bool opaque = source_prep_alpha_opaque(a.o), flip = a.o.y_flip != 0u;
    bool below = false;
    for (uint32_t y = blockIdx.y * SP_BLOCK_Y + threadIdx.y; y < a.height; y += gridDim.y * SP_BLOCK_Y) {
        const uint8_t* src_row = a.src + (size_t)source_row(y, a.height, flip) * a.src_pitch;
        uint8_t* dst_row = a.dst + (size_t)y * a.dst_pitch;
        for (uint32_t q = blockIdx.x * SP_BLOCK_X + threadIdx.x; q < quads; q += gridDim.x * SP_BLOCK_X) {
            const uint32_t x = q * 4u, n = min(4u, a.width - x);
            uint32_t v[4];
            load_quad(src_row + (size_t)x * 4u, n, v);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                v[k] = prepare_pixel(v[k], RENORM, a.o.swizzle, opaque);
                below |= k < n && (v[k] >> 24) < 255u;
            }
            store_quad(dst_row + (size_t)x * 4u, n, v);
        }
    }
    // every lane of the wave arrives here (no early return above); a wave is one row of the workgroup, so its first lane is threadIdx.x == 0
    if (__ballot(below) != 0ull && threadIdx.x == 0u && __hip_atomic_load(a.any_alpha, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(a.any_alpha, 1u);
}

__global__ __launch_bounds__(SP_BLOCK_X * SP_BLOCK_Y) void split_alpha_kernel(split_alpha_args a) {
    const uint32_t quads = (a.width + 3u) >> 2;
    for (uint32_t y = blockIdx.y * SP_BLOCK_Y + threadIdx.y; y < a.height; y += gridDim.y * SP_BLOCK_Y) {
        const uint8_t* src_row = a.src + (size_t)y * a.src_pitch;
        uint8_t *rgb_row = a.dst_rgb + (size_t)y * a.rgb_pitch, *a_row = a.dst_a + (size_t)y * a.a_pitch;
        for (uint32_t q = blockIdx.x * SP_BLOCK_X + threadIdx.x; q < quads; q += gridDim.x * SP_BLOCK_X) {
            const uint32_t x = q * 4u, n = min(4u, a.width - x);
            uint32_t v[4], rgb[4], al[4];
            load_quad(src_row + (size_t)x * 4u, n, v);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) { rgb[k] = split_alpha_rgb(v[k]); al[k] = split_alpha_a(v[k]); }
            store_quad(rgb_row + (size_t)x * 4u, n, rgb);
            store_quad(a_row + (size_t)x * 4u, n, al);
        }
    }
}

static dim3 grid_for(uint32_t width, uint32_t height) {
    const uint32_t quads = (width + 3u) >> 2;
    const uint32_t gx = std::min<uint32_t>((quads + SP_BLOCK_X - 1u) / SP_BLOCK_X, SP_MAX_GRID_X);
    return dim3(gx, std::min<uint32_t>((height + SP_BLOCK_Y - 1u) / SP_BLOCK_Y, SP_MAX_GRID / gx));
}

hipError_t launch_prepare_source(hipStream_t st, const source_prep_args& a) {
    static_assert(SP_BLOCK_X == 64, "a wave is one row of the workgroup");
    hipError_t e = hipMemsetAsync(a.any_alpha, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !a.width || !a.height) return e;
    with_bool(a.o.renormalize != 0u, [&](auto renorm) {
        hipLaunchKernelGGL((prepare_source_kernel<decltype(renorm)::value>), grid_for(a.width, a.height), dim3(SP_BLOCK_X, SP_BLOCK_Y), 0, st, a);
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_split_alpha(hipStream_t st, const split_alpha_args& a) {
    if (!a.width || !a.height) return hipSuccess;
    hipLaunchKernelGGL(split_alpha_kernel, grid_for(a.width, a.height), dim3(SP_BLOCK_X, SP_BLOCK_Y), 0, st, a);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace bu
