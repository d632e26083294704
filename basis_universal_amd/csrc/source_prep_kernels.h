// source_prep_kernels.h -- launchers of source_prep_kernels.hip: the per-pixel source preparation of basis_compressor::read_source_images and the ETC1S alpha split,
// over resident RGBA8 rasters (4-byte aligned, row pitches in bytes and multiples of 4, at most 16384 pixels each way: the callers check).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "source_prep.h"

namespace bu {

struct source_prep_args {
    const uint8_t* src;
    uint8_t* dst;            // may equal src unless o.y_flip is set
    uint32_t* any_alpha;     // device word: bit 0 is set where a prepared alpha value is below 255 (cleared by the launcher)
    uint32_t width, height, src_pitch, dst_pitch;
    source_prep_options o;
};

struct split_alpha_args {
    const uint8_t* src;
    uint8_t *dst_rgb, *dst_a;
    uint32_t width, height, src_pitch, rgb_pitch, a_pitch;
};

// one launch each
hipError_t launch_prepare_source(hipStream_t st, const source_prep_args& a);
hipError_t launch_split_alpha(hipStream_t st, const split_alpha_args& a);

}  // namespace bu
