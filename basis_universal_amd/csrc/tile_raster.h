// tile_raster.h -- what every entry that moves 4x4 tiles into or out of a raster shares: the geometry of one image, and (device code, for hipcc only) the slice
// lookup, the clamped row read and the cropped row / block stores behind the transcoders (uastc_transcode_kernels.hip, etc1s_transcode_kernels.hip), the DDS packers
// (dds_pack_kernels.hip) and the tilers (etc1s_misc_kernels.hip). The host half -- defaults, refusals, the slice table's pack -- is tile_geometry_check.h.
#pragma once
#include <stdint.h>
#include "../../include/basisu_hip.h"

namespace bu {

// One image as tiles and as pixels, every zero of the caller's replaced by what it stands for (resolve_geometry): nbx x nby tiles; width x height pixels
// (<= 4 * nbx, 4 * nby) are the image; the raster has `pitch` pixels per row and `rows` rows, and rows of the image past `rows` are not written.
struct tile_geometry {
    uint32_t nbx, nby, width, height, pitch, rows;
};

// mul_8 (transcoder.cpp:269): an 8-bit value scaled to q, and on it the three 16-bit pixel formats of both transcoders' pixel targets (transcoder.cpp:9155-9332,
// :10246-10302). Host and device: the UASTC core's host build packs the same pixels.
#ifdef __HIPCC__
#define BU_RASTER_FN __host__ __device__ __forceinline__
#else
#define BU_RASTER_FN static inline
#endif
BU_RASTER_FN uint32_t mul_8(uint32_t v, uint32_t q) { v = v * q + 128u; return ((v + (v >> 8)) >> 8) & 255u; }
BU_RASTER_FN uint32_t pack_rgb565(uint32_t r, uint32_t g, uint32_t b) { return (mul_8(r, 31) << 11) | (mul_8(g, 63) << 5) | mul_8(b, 31); }
BU_RASTER_FN uint32_t pack_rgba4444(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return (mul_8(r, 15) << 12) | (mul_8(g, 15) << 8) | (mul_8(b, 15) << 4) | mul_8(a, 15); }

}  // namespace bu

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace bu {

// The slice table: items (blocks, tiles) of all slices in table order, one or several lanes per item. `prefix` (n_slices + 1 entries, strictly ascending -- every
// slice has at least one item --, prefix[n_slices] = total) says where each slice's items begin in that order. The slice of a wave's first item is found once per
// wave by bisection at wave-uniform addresses (scalar loads through the scalar cache), and each lane steps on from there: at most 63 steps, where a wave covers
// one-item slices only. false: the lane has no item. Every lane of the wave must call it (the bisection reads the wave's first lane).
__device__ __forceinline__ bool find_slice(const uint32_t* __restrict__ prefix, uint32_t n_slices, uint32_t total, uint32_t item, uint32_t& slice, uint32_t& local) {
    const uint32_t wave_first = __builtin_amdgcn_readfirstlane(item);
    uint32_t lo = 0, hi = n_slices;                       // prefix[lo] <= wave_first < prefix[hi] while the wave has any item at all
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= wave_first) lo = mid; else hi = mid;
    }
    if (item >= total) return false;
    uint32_t s = lo;
    while (item >= prefix[s + 1u]) s++;                   // ends: item < total = prefix[n_slices]
    slice = s;
    local = item - prefix[s];
    return true;
}

// a record of the whole-file transcoders and the DDS pixel packer as the entry uploads it (slice_table, tile_geometry_check.h)
struct transcode_slice_view {
    uint64_t first_block, alpha_first_block, out_offset;
    tile_geometry g;
    uint32_t slice, local;   // the slice's index in the table, and the lane's block within the slice (raster order)
};

// find_slice with a lane per block, and the slice's record; false: the lane has no block. Every lane of the wave must call it.
__device__ __forceinline__ bool find_transcode_slice(const bu_hip_transcode_slice* __restrict__ slices, const uint32_t* __restrict__ prefix, uint32_t n_slices,
                                                     uint32_t total_blocks, uint32_t block, transcode_slice_view& v) {
    static_assert(sizeof(bu_hip_transcode_slice) == 48, "a record is read as three 16-byte words");
    if (!find_slice(prefix, n_slices, total_blocks, block, v.slice, v.local)) return false;
    const uint4* rec = reinterpret_cast<const uint4*>(slices + v.slice);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];    // { first_block lo, hi, alpha_first_block lo, hi } { out_offset lo, hi, nbx, nby } { width, height, pitch, rows }
    v.first_block = (uint64_t)r0.x | ((uint64_t)r0.y << 32);
    v.alpha_first_block = (uint64_t)r0.z | ((uint64_t)r0.w << 32);
    v.out_offset = (uint64_t)r1.x | ((uint64_t)r1.y << 32);
    v.g = tile_geometry{ r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
    return true;
}

// Row y of tile column bx of an RGBA8 raster (`pitch` in bytes), clamped at the right and bottom edge (image::extract_block_clamped): one 16-byte load where the
// row is whole and the raster aligned, else texel by texel.
__device__ __forceinline__ uint4 load_tile_row_clamped(const uint8_t* __restrict__ rgba, uint32_t pitch, uint32_t width, uint32_t height, uint32_t bx, uint32_t y) {
    const uint8_t* line = rgba + (size_t)min(y, height - 1u) * pitch;
    if (bx * 4u + 3u < width && ((pitch | (uint32_t)(uintptr_t)rgba) & 15u) == 0) return *reinterpret_cast<const uint4*>(line + (size_t)bx * 16u);
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t x = min(bx * 4u + (uint32_t)k, width - 1u);
        const uint8_t* q = line + (size_t)x * 4u;
        p[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    return make_uint4(p[0], p[1], p[2], p[3]);
}

// One row of tile column bx, four pixels of `unit` bytes (4, 2 or 1: a constant at every call site once inlined) in the low bits of v[], cropped to `width`. `dst`
// is where the tile's row begins: one 16 / 8 / 4-byte word where the row is whole and the address allows, else texel by texel.
__device__ __forceinline__ void store_tile_row(uint32_t unit, void* dst, uint32_t bx, uint32_t width, const uint32_t v[4]) {
    const bool whole = bx * 4u + 4u <= width;
    if (unit == 4) {
        if (whole && ((uintptr_t)dst & 15u) == 0) *(uint4*)dst = make_uint4(v[0], v[1], v[2], v[3]);
        else {
#pragma unroll
            for (uint32_t x = 0; x < 4; x++) if (bx * 4u + x < width) ((uint32_t*)dst)[x] = v[x];
        }
    } else if (unit == 2) {
        if (whole && ((uintptr_t)dst & 7u) == 0) *(uint2*)dst = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
        else {
#pragma unroll
            for (uint32_t x = 0; x < 4; x++) if (bx * 4u + x < width) ((uint16_t*)dst)[x] = (uint16_t)v[x];
        }
    } else {
        if (whole && ((uintptr_t)dst & 3u) == 0) *(uint32_t*)dst = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else {
#pragma unroll
            for (uint32_t x = 0; x < 4; x++) if (bx * 4u + x < width) ((uint8_t*)dst)[x] = (uint8_t)v[x];
        }
    }
}

// block i of a block target: w[0] as one uint2 at out[i], or both words as one uint4
__device__ __forceinline__ void store_block_words(void* out, uint32_t i, const uint64_t w[2], bool sixteen_bytes) {
    if (sixteen_bytes) ((uint4*)out)[i] = make_uint4((uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32));
    else ((uint2*)out)[i] = make_uint2((uint32_t)w[0], (uint32_t)(w[0] >> 32));
}

}  // namespace bu
#endif  // __HIPCC__
