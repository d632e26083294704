// mip_levels_kernels.hip -- caller-supplied mip levels (mip_levels.h) into tight RGBA8 rasters: every level of every image of a call in ONE launch.
// A chain below 20x28 is 10x14, 5x7, 2x3 and 1x1 pixels: a launch per level costs far more than the copy. One lane per pixel over the pixels of all records in table
// order; `prefix` (n_levels + 1 entries, strictly ascending, prefix[n_levels] = total) says where each record's pixels begin in that order, and find_slice
// (tile_raster.h) gives a lane its record as it gives k_extract_slices its slice: a bisection per wave, then at most 63 steps where a wave covers one-pixel levels.
// Per pixel: one dword load, one byte permute (v_perm_b32 with the record's selector: byte order and swizzle composed by the host), one dword store. Both sides are
// tight and 4-byte aligned, so a wave moves 256 contiguous bytes each way. No LDS, no scratch.
// "Any written alpha is not 255" is kept per record: the lanes of a wave that saw one are grouped by record with a ballot, and the first lane of each group does one
// vector atomicOr on that record's word -- unless a relaxed load shows the bit already set, as in source_prep_kernels.hip.
#include <hip/hip_runtime.h>
#include "launch_dispatch.h"
#include "mip_levels.h"

namespace bu {

__global__ __launch_bounds__(256) void k_prepare_mip_levels(const uint8_t* __restrict__ payload, const bu_hip_mip_level_record* __restrict__ records,
                                                            const uint32_t* __restrict__ prefix, uint32_t n_levels, uint32_t total, uint8_t* __restrict__ out,
                                                            uint32_t* __restrict__ flags) {
    const uint32_t pixel = blockIdx.x * 256u + threadIdx.x;   // total <= 2^30 (the table's builder refuses more)
    uint32_t level = 0, local = 0;
    bool below = false;
    if (find_slice(prefix, n_levels, total, pixel, level, local)) {   // every lane of the wave calls it
        const uint4* rec = reinterpret_cast<const uint4*>(records + level);
        const uint4 r0 = rec[0], r1 = rec[1];             // { src_offset lo, hi, dst_offset lo, hi } { width, height, selector, reserved }
        const uint64_t src = ((uint64_t)r0.x | ((uint64_t)r0.y << 32)) + (uint64_t)local * 4u, dst = ((uint64_t)r0.z | ((uint64_t)r0.w << 32)) + (uint64_t)local * 4u;
        const uint32_t v = __builtin_amdgcn_perm(0u, *reinterpret_cast<const uint32_t*>(payload + src), r1.z);   // selector bytes 0..3 pick from the second operand
        *reinterpret_cast<uint32_t*>(out + dst) = v;
        below = (v >> 24) != 255u;
    }
    // every lane of the wave arrives here; the loop's condition is wave-uniform and each turn retires the lanes of one record
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t pending = __ballot(below); pending != 0ull;) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)pending) - 1u;
        const uint32_t its_level = (uint32_t)__shfl((int)level, (int)leader);
        const bool mine = below && level == its_level;
        if (lane == leader && __hip_atomic_load(flags + its_level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(flags + its_level, 1u);
        pending &= ~__ballot(mine);
    }
}

hipError_t launch_prepare_mip_levels(hipStream_t st, const void* d_payload, const bu_hip_mip_level_record* d_records, const uint32_t* d_prefix, uint32_t n_levels,
                                     uint32_t total_pixels, void* d_out, uint32_t* d_flags) {
    if (!n_levels || !total_pixels) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d_flags, 0, (size_t)n_levels * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_prepare_mip_levels, dim3((total_pixels + 255u) / 256u), dim3(256), 0, st, static_cast<const uint8_t*>(d_payload), d_records, d_prefix, n_levels,
                       total_pixels, static_cast<uint8_t*>(d_out), d_flags);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace bu
