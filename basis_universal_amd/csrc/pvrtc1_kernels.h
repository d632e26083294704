// pvrtc1_kernels.h -- launchers of pvrtc1_kernels.hip: resident ETC1S palettes + indices, or resident UASTC blocks, to PVRTC1 4bpp RGB / RGBA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/basisu_hip.h"

namespace bu {

// the four routes: which codec the blocks are in, and whether the texture carries alpha
enum pvrtc1_source : uint32_t { PVRTC1_FROM_ETC1S_RGB = 0, PVRTC1_FROM_ETC1S_RGBA = 1, PVRTC1_FROM_UASTC_RGB = 2, PVRTC1_FROM_UASTC_RGBA = 3 };

// One image (n_slices == 0: nbx x nby blocks, the index arrays / the blocks are the image's own) or every image of a file (a slice table as the whole-file
// transcoders upload it: first_block / alpha_first_block count entries of endpoint_idx / selector_idx, or blocks of `blocks`).
struct pvrtc1_args {
    const uint32_t *endpoint_palette, *selector_palette;   // ETC1S, as etc1s_transcode_args has them
    const uint16_t *endpoint_idx, *selector_idx, *alpha_endpoint_idx, *alpha_selector_idx;   // one image: the alpha slice's own arrays (RGBA route only)
    const uint4* blocks;                                   // UASTC
    uint32_t* words;                                       // the workspace between the passes: total_blocks endpoint words, images back to back in raster order
    uint8_t* out;                                          // image s writes nbx * nby * 8 bytes at out + out_offset (one image: at out)
    uint32_t* invalid;                                     // one counter, or n_slices
    const bu_hip_transcode_slice* slices;
    const uint32_t* prefix;
    uint32_t n_slices, total_blocks, n_endpoints, n_selectors, nbx, nby;
};

// Both passes, queued back to back on `st`: the counters are cleared first and afterwards hold how many blocks were invalid (written as eight zero bytes).
// Every image must be a power of two blocks each way; the caller has checked that, and that `words` has room for total_blocks words.
hipError_t launch_transcode_pvrtc1(hipStream_t st, const pvrtc1_args& a, pvrtc1_source source);

}  // namespace bu
