// mip_levels.h -- mip levels the caller made (basis_compressor_params::m_source_mipmap_images, comp.cpp:2737-2818; the levels of a .dds source,
// read_uncompressed_dds_file, gpu_texture.cpp:2025-2210) brought into tight RGBA8 rasters: every level of every image of a call from ONE resident payload in ONE launch.
// What the reference does to such a level is a byte permutation per pixel -- the R/B swap of a B8G8R8A8 file, then the swizzle; renormalise, flip, alpha policy and
// resample touch level 0 only --, so a level's record carries the two composed into one selector word, and level 0 of a .dds source the byte order alone.
// The host half (plain C++: the record checks and the pack, as tile_geometry_check.h has them for the other tables) and the launcher of mip_levels_kernels.hip.
#pragma once
#include "tile_geometry_check.h"

namespace bu {

enum : uint32_t { MIP_LEVELS_MAX_DIMENSION = 16384u, MIP_LEVELS_MAX_RECORDS = 0xFFFFFFu };   // BASISU_MAX_SUPPORTED_TEXTURE_DIMENSION, BASISU_MAX_SLICES

// byte i of the word names the source byte (0..3) of output channel i
inline bool mip_level_selector_valid(uint32_t selector) { return (selector & 0xFCFCFCFCu) == 0u; }

// Every refusal of a table of bu_hip_mip_level_record, and the pack: the records as they are, a level's items are its pixels. Nothing else is touched.
inline int build_mip_level_records(slice_table& t, const char* fn, const void* d_payload, size_t payload_bytes, const bu_hip_mip_level_record* records, uint32_t n,
                                   const void* d_out, size_t out_bytes, const void* d_flags, err_text err) {
    static_assert(sizeof(bu_hip_mip_level_record) == 32, "the kernel reads a record as two 16-byte words");
    if (!d_payload || !records || !d_out || !d_flags) return refuse(err, "%s: null pointer", fn);
    if (((uintptr_t)d_payload | (uintptr_t)d_out | (uintptr_t)d_flags) & 3u) return refuse(err, "%s: the payload, the output and the flags must be 4-byte aligned", fn);
    if (n > MIP_LEVELS_MAX_RECORDS) return refuse(err, "%s: %u records are more than the %u slices of one file", fn, n, (uint32_t)MIP_LEVELS_MAX_RECORDS);
    t.begin(n, sizeof(bu_hip_mip_level_record), false);
    for (uint32_t i = 0; i < n; i++) {
        const bu_hip_mip_level_record& r = records[i];
        if (!r.width || !r.height || r.width > MIP_LEVELS_MAX_DIMENSION || r.height > MIP_LEVELS_MAX_DIMENSION)
            return refuse(err, "%s: level %u: %u x %u pixels (1..%u each way)", fn, i, r.width, r.height, (uint32_t)MIP_LEVELS_MAX_DIMENSION);
        if ((r.src_offset | r.dst_offset) & 3u)
            return refuse(err, "%s: level %u: src_offset %llu / dst_offset %llu is not 4-byte aligned", fn, i, (ull)r.src_offset, (ull)r.dst_offset);
        if (!mip_level_selector_valid(r.selector)) return refuse(err, "%s: level %u: selector entry above 3 (0x%08x; one byte per channel, each 0..3)", fn, i, r.selector);
        const uint64_t bytes = (uint64_t)r.width * r.height * 4u;
        if (r.src_offset > payload_bytes || bytes > payload_bytes - r.src_offset)
            return refuse(err, "%s: level %u: its source, bytes %llu..%llu, ends past payload_bytes = %llu", fn, i, (ull)r.src_offset, (ull)(r.src_offset + bytes), (ull)payload_bytes);
        if (r.dst_offset > out_bytes || bytes > out_bytes - r.dst_offset)
            return refuse(err, "%s: level %u: its raster, bytes %llu..%llu, ends past out_bytes = %llu", fn, i, (ull)r.dst_offset, (ull)(r.dst_offset + bytes), (ull)out_bytes);
        if (!t.add(fn, i, &r, bytes / 4u, "pixels", err)) return 0;
    }
    return 1;
}

}  // namespace bu

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace bu {

// One launch (and the clearing of the n flag words in front of it) on `st`; n_levels == 0 does nothing. d_records / d_prefix: the uploaded pack of build_mip_level_records.
hipError_t launch_prepare_mip_levels(hipStream_t st, const void* d_payload, const bu_hip_mip_level_record* d_records, const uint32_t* d_prefix, uint32_t n_levels,
                                     uint32_t total_pixels, void* d_out, uint32_t* d_flags);

}  // namespace bu
#endif
