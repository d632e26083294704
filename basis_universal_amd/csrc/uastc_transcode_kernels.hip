// uastc_transcode_kernels.hip -- basisu_lowlevel_uastc_ldr_4x4_transcoder::transcode_slice (transcoder/basisu_transcoder.cpp:10078-10339) over resident UASTC
// blocks: one lane per 16-byte block, the target a template parameter so that each instance carries only its own path (uastc_transcode.h). A block
// is loaded as one uint4 and its result stored as whole uint2 / uint4 words, consecutive lanes on consecutive blocks; RGBA32 writes the four 16-byte
// rows of its tile into the caller's raster, cropped to the image. A block the core refuses (mode code that matches nothing, pattern index out of
// range) gets zeros and is counted with a vector atomic; it never stops the others. Two kernels share that per-block work: one image per launch, and every
// image of a file in one launch through a slice table (tile_raster.h), counted per slice.
#include <hip/hip_runtime.h>
#include "uastc_transcode.h"
#include "uastc_transcode_kernels.h"
#include "tile_raster.h"
#include "tile_geometry_check.h"

namespace bu {
using namespace bu_uastc;

struct transcode_args {
    const uint4* blocks;
    void* out;
    uint32_t* invalid;
    tile_geometry g;
    uint32_t chan0, chan1;
};

// One block: unpack, the target's conversion, the store. `out` is where the image's output begins, `i` the block's place in the image's raster order. RGBA32
// writes the four rows of the tile cropped to width x min(height, rows) (store_tile_row); every other target one uint2 / uint4 at out[i] (store_block_words).
// false = the block did not unpack and zeros were written. Both kernels below are this function behind their own indexing.
template <uint32_t TARGET, bool HQ>
__device__ __forceinline__ bool transcode_uastc_block(const uint4 in, void* out, uint32_t i, const tile_geometry& g, uint32_t chan0, uint32_t chan1) {
    uint8_t blk[16];
    const uint32_t words[4] = { in.x, in.y, in.z, in.w };
    BU_UNROLL
    for (int k = 0; k < 16; k++) blk[k] = (uint8_t)(words[k >> 2] >> (8 * (k & 3)));
    bool ok;
    if (TARGET == TF_RGBA32) {
        rgba8 px[16];
        ok = transcode_rgba32(blk, px);
        const uint32_t bx = i % g.nbx, by = i / g.nbx;
        BU_UNROLL
        for (uint32_t y = 0; y < 4; y++) {
            const uint32_t row = by * 4 + y;
            if (row >= g.height || row >= g.rows) break;
            uint32_t v[4];
            BU_UNROLL
            for (uint32_t x = 0; x < 4; x++) v[x] = ok ? pack_px(px[y * 4 + x].c) : 0u;
            store_tile_row(4, (uint32_t*)out + (size_t)row * g.pitch + bx * 4, bx, g.width, v);
        }
    } else if (TARGET == TF_ASTC_4x4_RGBA || TARGET == TF_BC7_RGBA) {
        uint8_t o[16];
        ok = TARGET == TF_BC7_RGBA ? transcode_bc7(blk, o) : transcode_astc(blk, o);
        uint32_t w[4] = { 0, 0, 0, 0 };
        if (ok) {
            BU_UNROLL
            for (int k = 0; k < 16; k++) w[k >> 2] |= (uint32_t)o[k] << (8 * (k & 3));
        }
        ((uint4*)out)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (TARGET == TF_RGB565 || TARGET == TF_BGR565 || TARGET == TF_RGBA4444) {   // the texture family's 16-bit rasters: RGBA32's tile walk with 2-byte pixels
        rgba8 px[16];
        ok = transcode_rgba32(blk, px);
        const uint32_t bx = i % g.nbx, by = i / g.nbx;
        BU_UNROLL
        for (uint32_t y = 0; y < 4; y++) {
            const uint32_t row = by * 4 + y;
            if (row >= g.height || row >= g.rows) break;
            uint32_t v[4];
            BU_UNROLL
            for (uint32_t x = 0; x < 4; x++) v[x] = ok ? pack_pixel16<TARGET>(px[y * 4 + x]) : 0u;
            store_tile_row(2, (uint16_t*)out + (size_t)row * g.pitch + bx * 4, bx, g.width, v);
        }
    } else if (TARGET == TF_ETC1_RGB || TARGET == TF_ETC2_RGBA || TARGET == TF_ETC2_EAC_R11 || TARGET == TF_ETC2_EAC_RG11) {   // the texture family's block targets
        uint64_t w[2] = { 0, 0 };
        ok = transcode_etc<TARGET, HQ>(blk, chan0, chan1, w);
        if (!ok) w[0] = w[1] = 0;
        store_block_words(out, i, w, TARGET == TF_ETC2_RGBA || TARGET == TF_ETC2_EAC_RG11);
    } else {
        uint64_t w[2] = { 0, 0 };
        ok = transcode_bcn(blk, TARGET, HQ, chan0, chan1, w);
        if (!ok) w[0] = w[1] = 0;
        store_block_words(out, i, w, !(TARGET == TF_BC1_RGB || TARGET == TF_BC4_R));
    }
    return ok;
}

template <uint32_t TARGET, bool HQ>
__global__ __launch_bounds__(256) void transcode_uastc_kernel(transcode_args a) {
    const uint32_t n = a.g.nbx * a.g.nby, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (!transcode_uastc_block<TARGET, HQ>(a.blocks[i], a.out, i, a.g, a.chan0, a.chan1)) atomicAdd(a.invalid, 1u);
}

// every image of a file in one launch (bu_hip_k_transcode_uastc_slices): find_transcode_slice (tile_raster.h) in front of the same block function
struct transcode_slices_args {
    const uint4* blocks;
    uint8_t* out;
    uint32_t* invalid;                      // n_slices counters
    const bu_hip_transcode_slice* slices;   // as the entry normalised them
    const uint32_t* prefix;
    uint32_t n_slices, total_blocks, chan0, chan1;
};

template <uint32_t TARGET, bool HQ>
__global__ __launch_bounds__(256) void transcode_uastc_slices_kernel(transcode_slices_args a) {
    transcode_slice_view v;
    if (!find_transcode_slice(a.slices, a.prefix, a.n_slices, a.total_blocks, blockIdx.x * 256u + threadIdx.x, v)) return;
    if (!transcode_uastc_block<TARGET, HQ>(a.blocks[v.first_block + v.local], a.out + v.out_offset, v.local, v.g, a.chan0, a.chan1)) atomicAdd(a.invalid + v.slice, 1u);
}

template <uint32_t TARGET, bool HQ>
static hipError_t launch(hipStream_t st, const transcode_args& a) {
    const uint32_t n = a.g.nbx * a.g.nby;
    hipLaunchKernelGGL((transcode_uastc_kernel<TARGET, HQ>), dim3((n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
template <uint32_t TARGET, bool HQ>
static hipError_t launch(hipStream_t st, const transcode_slices_args& a) {
    hipLaunchKernelGGL((transcode_uastc_slices_kernel<TARGET, HQ>), dim3((a.total_blocks + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// the instance of either kernel for (target, high_quality)
template <class Args>
static hipError_t launch_for_target(hipStream_t st, const Args& a, uint32_t target, bool high_quality) {
    switch (target) {
    case TF_RGBA32: return launch<TF_RGBA32, false>(st, a);
    case TF_ASTC_4x4_RGBA: return launch<TF_ASTC_4x4_RGBA, false>(st, a);
    case TF_BC7_RGBA: return launch<TF_BC7_RGBA, false>(st, a);
    case TF_BC1_RGB: return high_quality ? launch<TF_BC1_RGB, true>(st, a) : launch<TF_BC1_RGB, false>(st, a);
    case TF_BC3_RGBA: return high_quality ? launch<TF_BC3_RGBA, true>(st, a) : launch<TF_BC3_RGBA, false>(st, a);
    case TF_BC4_R: return launch<TF_BC4_R, false>(st, a);
    case TF_BC5_RG: return launch<TF_BC5_RG, false>(st, a);
    default: return hipErrorInvalidValue;
    }
}

// the texture family (bu_hip_k_transcode_uastc_texture / _textures): the seven targets above through the same instances, and its own -- high quality is a
// template parameter of R11 / RG11 only, whose packers it selects
template <class Args>
static hipError_t launch_for_texture_target(hipStream_t st, const Args& a, uint32_t target, bool high_quality) {
    switch (target) {
    case TF_ETC1_RGB: return launch<TF_ETC1_RGB, false>(st, a);
    case TF_ETC2_RGBA: return launch<TF_ETC2_RGBA, false>(st, a);
    case TF_ETC2_EAC_R11: return high_quality ? launch<TF_ETC2_EAC_R11, true>(st, a) : launch<TF_ETC2_EAC_R11, false>(st, a);
    case TF_ETC2_EAC_RG11: return high_quality ? launch<TF_ETC2_EAC_RG11, true>(st, a) : launch<TF_ETC2_EAC_RG11, false>(st, a);
    case TF_RGB565: return launch<TF_RGB565, false>(st, a);
    case TF_BGR565: return launch<TF_BGR565, false>(st, a);
    case TF_RGBA4444: return launch<TF_RGBA4444, false>(st, a);
    default: return launch_for_target(st, a, target, high_quality);
    }
}

size_t transcode_output_bytes(uint32_t nbx, uint32_t nby, uint32_t width, uint32_t height, uint32_t target) {
    const uint32_t bpb = transcode_bytes_per_block(target);
    if (!bpb) return 0;
    const bool pixels = target == TF_RGBA32;   // bpb is per block: 16 pixels of 4 bytes
    return raster_output_bytes(tile_geometry{ nbx, nby, width, height, 0, 0 }, pixels ? 4 : bpb, pixels);
}

uint32_t uastc_texture_unit_bytes(uint32_t target) { return texture_unit_bytes(target); }
bool uastc_texture_is_pixel_target(uint32_t target) { return texture_is_pixel_target(target); }

hipError_t launch_transcode_uastc(hipStream_t st, const void* d_blocks, const tile_geometry& g, uint32_t target, bool high_quality, uint32_t chan0, uint32_t chan1,
                                  void* d_out, uint32_t* d_invalid, bool texture_family) {
    transcode_args a = { (const uint4*)d_blocks, d_out, d_invalid, g, chan0, chan1 };
    hipError_t e = hipMemsetAsync(d_invalid, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !g.nbx || !g.nby) return e;
    return texture_family ? launch_for_texture_target(st, a, target, high_quality) : launch_for_target(st, a, target, high_quality);
}

hipError_t launch_transcode_uastc_slices(hipStream_t st, const void* d_blocks, const bu_hip_transcode_slice* d_slices, const uint32_t* d_prefix, uint32_t n_slices,
                                         uint32_t total_blocks, uint32_t target, bool high_quality, uint32_t chan0, uint32_t chan1, void* d_out, uint32_t* d_invalid,
                                         bool texture_family) {
    transcode_slices_args a = { (const uint4*)d_blocks, (uint8_t*)d_out, d_invalid, d_slices, d_prefix, n_slices, total_blocks, chan0, chan1 };
    hipError_t e = hipMemsetAsync(d_invalid, 0, (size_t)n_slices * sizeof(uint32_t), st);
    if (e != hipSuccess || !n_slices || !total_blocks) return e;
    return texture_family ? launch_for_texture_target(st, a, target, high_quality) : launch_for_target(st, a, target, high_quality);
}

} // namespace bu
