// transcode_slices.h -- the slice table both whole-file transcoders walk (bu_hip_k_transcode_uastc_slices, bu_hip_k_transcode_etc1s_slices): device code shared by
// uastc_transcode_kernels.hip and etc1s_transcode_kernels.hip.
// One lane per block over the blocks of all slices in table order. `prefix` (n_slices + 1 entries, strictly ascending -- every slice has at least one block --,
// prefix[n_slices] = total_blocks) says where each slice's blocks begin in that order. The slice of a wave's first block is found once per wave by bisection at
// wave-uniform addresses (scalar loads through the scalar cache), and each lane steps on from there: at most 63 steps, where a wave covers one-block slices only.
// This is k_extract_slices' lookup (etc1s_misc_kernels.hip) with a lane per block instead of a lane per block row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/basisu_hip.h"

namespace bu {

// a record as the entry uploads it: the caller's, with the sizes' zeros replaced by what they stand for (width / height: 4 * num_blocks; pitch / rows: width / height)
struct transcode_slice_view {
    uint64_t first_block, alpha_first_block, out_offset;
    uint32_t nbx, nby, width, height, pitch, rows;
    uint32_t slice, local;   // the slice's index in the table, and the lane's block within the slice (raster order)
};

// false: the lane has no block. Every lane of the wave must call it (the bisection reads the wave's first lane).
__device__ __forceinline__ bool find_transcode_slice(const bu_hip_transcode_slice* __restrict__ slices, const uint32_t* __restrict__ prefix, uint32_t n_slices,
                                                     uint32_t total_blocks, uint32_t block, transcode_slice_view& v) {
    static_assert(sizeof(bu_hip_transcode_slice) == 48, "a record is read as three 16-byte words");
    const uint32_t wave_first = __builtin_amdgcn_readfirstlane(block);
    uint32_t lo = 0, hi = n_slices;                       // prefix[lo] <= wave_first < prefix[hi] while the wave has any block at all
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= wave_first) lo = mid; else hi = mid;
    }
    if (block >= total_blocks) return false;
    uint32_t s = lo;
    while (block >= prefix[s + 1u]) s++;                  // ends: block < total_blocks = prefix[n_slices]
    const uint4* rec = reinterpret_cast<const uint4*>(slices + s);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];    // { first_block lo, hi, alpha_first_block lo, hi } { out_offset lo, hi, nbx, nby } { width, height, pitch, rows }
    v.first_block = (uint64_t)r0.x | ((uint64_t)r0.y << 32);
    v.alpha_first_block = (uint64_t)r0.z | ((uint64_t)r0.w << 32);
    v.out_offset = (uint64_t)r1.x | ((uint64_t)r1.y << 32);
    v.nbx = r1.z; v.nby = r1.w; v.width = r2.x; v.height = r2.y; v.pitch = r2.z; v.rows = r2.w;
    v.slice = s;
    v.local = block - prefix[s];
    return true;
}

}  // namespace bu
