// pvrtc1_kernels.hip -- PVRTC1 4bpp RGB / RGBA from resident ETC1S palettes + indices and from resident UASTC blocks (pvrtc1.h): the one target whose block
// depends on its neighbours, so two kernels per call, queued back to back on the caller's stream with no host wait between them.
//   endpoints   one lane per block writes the block's 32-bit endpoint word to a workspace of 4 bytes per block, in raster order
//   modulation  one lane per block reads the nine words of the 3x3 blocks around it (wrapped at the image's edges), derives its 16 texel values from its own source
//               block again, and stores one uint2 (modulation, endpoints) at the block's Morton address
// Both are templates over the four routes (ETC1S / UASTC, RGB / RGBA) and serve one image or every image of a file through a slice table (tile_raster.h): the
// lookup of the lane's image is the only difference. An invalid block (an ETC1S index past its palette, a UASTC block that does not unpack) gets the word 0 in
// the first pass, which its neighbours read as it stands; the second pass stores eight zero bytes for it and counts it with a vector atomic, per slice.
#include <hip/hip_runtime.h>
#include "uastc_transcode.h"
#include "pvrtc1.h"
#include "pvrtc1_kernels.h"
#include "tile_raster.h"

namespace bu {
using namespace bu_pvrtc1;

// the image a lane works in, and its block there
struct pvrtc1_view {
    const uint16_t *endpoint_idx, *selector_idx, *alpha_endpoint_idx, *alpha_selector_idx;   // the image's own
    const uint4* blocks;
    uint32_t* words;
    uint2* out;
    uint32_t nbx, nby, local, slice;
};

// false: the lane has no block. Every lane of the wave must call it (find_transcode_slice).
__device__ __forceinline__ bool pvrtc1_find(const pvrtc1_args& a, uint32_t item, pvrtc1_view& v) {
    if (a.n_slices == 0) {
        if (item >= a.total_blocks) return false;
        v = pvrtc1_view{ a.endpoint_idx, a.selector_idx, a.alpha_endpoint_idx, a.alpha_selector_idx, a.blocks, a.words, (uint2*)a.out, a.nbx, a.nby, item, 0u };
        return true;
    }
    transcode_slice_view s;
    if (!find_transcode_slice(a.slices, a.prefix, a.n_slices, a.total_blocks, item, s)) return false;
    const bool alpha = s.alpha_first_block != BU_HIP_NO_ALPHA_SLICE;
    v = pvrtc1_view{ a.endpoint_idx + s.first_block, a.selector_idx + s.first_block, alpha ? a.endpoint_idx + s.alpha_first_block : nullptr,
                     alpha ? a.selector_idx + s.alpha_first_block : nullptr, a.blocks + s.first_block, a.words + (item - s.local), (uint2*)(a.out + s.out_offset),
                     s.g.nbx, s.g.nby, s.local, s.slice };
    return true;
}

// what a lane has of its own block: the palette words (ETC1S) or the 16 pixels (UASTC). false: the block is invalid and nothing was gathered.
template <uint32_t SOURCE>
struct pvrtc1_block {
    uint32_t entry, sel, alpha_entry, alpha_sel, px[16];
};
template <uint32_t SOURCE>
__device__ __forceinline__ bool pvrtc1_load(const pvrtc1_args& a, const pvrtc1_view& v, pvrtc1_block<SOURCE>& b) {
    if (SOURCE == PVRTC1_FROM_ETC1S_RGB || SOURCE == PVRTC1_FROM_ETC1S_RGBA) {
        const uint32_t ei = v.endpoint_idx[v.local], si = v.selector_idx[v.local];
        bool ok = ei < a.n_endpoints && si < a.n_selectors;
        uint32_t aei = 0, asi = 0;
        if (SOURCE == PVRTC1_FROM_ETC1S_RGBA) {
            aei = v.alpha_endpoint_idx[v.local]; asi = v.alpha_selector_idx[v.local];
            ok = ok && aei < a.n_endpoints && asi < a.n_selectors;
        }
        if (!ok) return false;
        b.entry = a.endpoint_palette[ei]; b.sel = a.selector_palette[si];
        b.alpha_entry = b.alpha_sel = 0;
        if (SOURCE == PVRTC1_FROM_ETC1S_RGBA) { b.alpha_entry = a.endpoint_palette[aei]; b.alpha_sel = a.selector_palette[asi]; }
        return true;
    } else {
        const uint4 in = v.blocks[v.local];
        const uint32_t w[4] = { in.x, in.y, in.z, in.w };
        uint8_t blk[16];
        BU_UNROLL
        for (int k = 0; k < 16; k++) blk[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        bu_uastc::rgba8 px[16];
        if (!bu_uastc::transcode_rgba32(blk, px)) return false;
        BU_UNROLL
        for (int k = 0; k < 16; k++) b.px[k] = bu_uastc::pack_px(px[k].c);
        return true;
    }
}

template <uint32_t SOURCE>
__global__ __launch_bounds__(256) void pvrtc1_endpoints_kernel(pvrtc1_args a) {
    constexpr bool kAlpha = SOURCE == PVRTC1_FROM_ETC1S_RGBA || SOURCE == PVRTC1_FROM_UASTC_RGBA;
    pvrtc1_view v;
    if (!pvrtc1_find(a, blockIdx.x * 256u + threadIdx.x, v)) return;
    pvrtc1_block<SOURCE> b;
    uint32_t word = 0;
    if (pvrtc1_load<SOURCE>(a, v, b))
        word = (SOURCE == PVRTC1_FROM_ETC1S_RGB || SOURCE == PVRTC1_FROM_ETC1S_RGBA) ? etc1s_endpoint_word<kAlpha>(b.entry, b.sel, b.alpha_entry, b.alpha_sel)
                                                                                       : pixels_endpoint_word<kAlpha>(b.px);
    v.words[v.local] = word;
}

template <uint32_t SOURCE>
__global__ __launch_bounds__(256) void pvrtc1_modulation_kernel(pvrtc1_args a) {
    constexpr bool kAlpha = SOURCE == PVRTC1_FROM_ETC1S_RGBA || SOURCE == PVRTC1_FROM_UASTC_RGBA;
    pvrtc1_view v;
    if (!pvrtc1_find(a, blockIdx.x * 256u + threadIdx.x, v)) return;
    const uint32_t x = v.local & (v.nbx - 1u), y = v.local >> log2_pow2(v.nbx);   // both sizes are powers of two
    uint32_t words[9];
    BU_UNROLL
    for (uint32_t ey = 0; ey < 3; ey++) {
        const uint32_t* row = v.words + (size_t)((y + ey - 1u) & (v.nby - 1u)) * v.nbx;
        BU_UNROLL
        for (uint32_t ex = 0; ex < 3; ex++) words[ey * 3 + ex] = row[(x + ex - 1u) & (v.nbx - 1u)];
    }
    pvrtc1_block<SOURCE> b;
    uint2 o = make_uint2(0u, 0u);
    const bool ok = pvrtc1_load<SOURCE>(a, v, b);
    if (ok) {
        int cl[16];
        if (SOURCE == PVRTC1_FROM_ETC1S_RGB || SOURCE == PVRTC1_FROM_ETC1S_RGBA) etc1s_texel_values<kAlpha>(b.entry, b.sel, b.alpha_entry, b.alpha_sel, cl);
        else pixels_texel_values<kAlpha>(b.px, cl);
        o = make_uint2(modulation<kAlpha>(words, cl), words[4]);
    }
    v.out[morton_address(x, y, v.nbx, v.nby)] = o;
    if (!ok) atomicAdd(a.invalid + v.slice, 1u);
}

template <uint32_t SOURCE>
static hipError_t launch_both(hipStream_t st, const pvrtc1_args& a) {
    const dim3 grid((a.total_blocks + 255u) / 256u), block(256);
    hipLaunchKernelGGL((pvrtc1_endpoints_kernel<SOURCE>), grid, block, 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pvrtc1_modulation_kernel<SOURCE>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_transcode_pvrtc1(hipStream_t st, const pvrtc1_args& a, pvrtc1_source source) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, (size_t)(a.n_slices ? a.n_slices : 1u) * sizeof(uint32_t), st);
    if (e != hipSuccess || !a.total_blocks) return e;
    switch (source) {
    case PVRTC1_FROM_ETC1S_RGB: return launch_both<PVRTC1_FROM_ETC1S_RGB>(st, a);
    case PVRTC1_FROM_ETC1S_RGBA: return launch_both<PVRTC1_FROM_ETC1S_RGBA>(st, a);
    case PVRTC1_FROM_UASTC_RGB: return launch_both<PVRTC1_FROM_UASTC_RGB>(st, a);
    case PVRTC1_FROM_UASTC_RGBA: return launch_both<PVRTC1_FROM_UASTC_RGBA>(st, a);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace bu
