// etc1s_transcode_kernels.h -- launchers of etc1s_transcode_kernels.hip: the device half of reading an ETC1S file (palettes + per-block indices -> texture).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/basisu_hip.h"
#include "tile_raster.h"

namespace bu {

enum : uint32_t { kBc1TableEntries = 8 * 32 * 6 * 10 };   // per endpoint width: intensity tables x 5-bit base values x selector ranges x selector mappings
// the reference's transcoder_texture_format values of the targets that exist here
enum : uint32_t { ETF_ETC1_RGB = 0, ETF_ETC2_RGBA = 1, ETF_BC1_RGB = 2, ETF_BC7_RGBA = 6, ETF_ASTC_4x4_RGBA = 10, ETF_RGBA32 = 13, ETF_RGB565 = 14, ETF_BGR565 = 15, ETF_RGBA4444 = 16,
                  ETF_ETC2_EAC_R11 = 20, ETF_ETC2_EAC_RG11 = 21, ETF_ATC_RGB = 11, ETF_FXT1_RGB = 17, ETF_PVRTC2_4_RGB = 18, ETF_PVRTC2_4_RGBA = 19 };
enum : uint32_t { kEtc1sBc7TableWords = 8 * 32 * 6 * 10 + 128 };   // the ETC1S -> BC7 colour look-up and the mode-5 encoder's midpoints (etc1s_texture_targets.h)
enum : uint32_t { kEtc1sAtcTableWords = 3 * 8 * 32 * 6 * 10 };   // the three ETC1S -> ATC / PVRTC2 look-ups 55, 56, 45 (etc1s_vendor_format_targets.h)
enum : uint32_t { kEtc1sAstcTableWords = 2 * 8 * 32 * 6 * 10 + 48 };   // the two ETC1S -> ASTC look-ups and the 48 unquantised endpoint values (etc1s_block_format_targets.h)

struct etc1s_transcode_args {
    const uint32_t* endpoint_palette;   // r5 | g5 << 8 | b5 << 16 | intensity table << 24
    const uint32_t* selector_palette;   // selector of texel (x, y) at bits 2 * (y * 4 + x)
    const uint16_t *endpoint_idx, *selector_idx, *alpha_endpoint_idx, *alpha_selector_idx;   // alpha: both null = opaque
    void* out;
    uint32_t* invalid;                  // device counter
    const uint32_t* bc1_endpoints;      // BC1 only: 2 * kBc1TableEntries words from launch_etc1s_build_bc1_tables
    const uint32_t* bc7_tables;         // BC7 only: kEtc1sBc7TableWords words from launch_etc1s_build_bc7_tables
    uint32_t n_endpoints, n_selectors;
    tile_geometry g;
    const uint32_t* astc_tables;        // ASTC only: kEtc1sAstcTableWords words from launch_etc1s_build_astc_tables
};

// every image of a file in one launch: the file's two whole index arrays, and a table that says which ranges of them are whose
struct etc1s_transcode_slices_args {
    const uint32_t *endpoint_palette, *selector_palette;
    const uint16_t *endpoint_idx, *selector_idx;   // slice s reads [first_block, first_block + nbx * nby) of both, its alpha slice the same from alpha_first_block
    uint8_t* out;                                  // slice s writes at out + out_offset
    uint32_t* invalid;                             // n_slices device counters
    const uint32_t *bc1_endpoints, *bc7_tables;
    const bu_hip_transcode_slice* slices;          // device copies of the records, every zero size replaced by what it stands for
    const uint32_t* prefix;                        // n_slices + 1 entries: where each slice's blocks begin among the total_blocks of the call
    uint32_t n_endpoints, n_selectors, n_slices, total_blocks;
    const uint32_t* astc_tables;
};

uint32_t etc1s_transcode_unit_bytes(uint32_t target);   // per block for block targets, per pixel for pixel targets; 0 = not a target of the first six (ETC1, BC1, pixels)
uint32_t etc1s_texture_unit_bytes(uint32_t target);     // the same over all eight targets: also 16 for ETC2 RGBA and BC7 RGBA
uint32_t etc1s_block_format_unit_bytes(uint32_t target);   // the same over all eleven: also 16 for ASTC 4x4 and EAC RG11, 8 for EAC R11
uint32_t etc1s_vendor_format_unit_bytes(uint32_t target);  // the fourth family: also 8 for ATC RGB and PVRTC2 4bpp RGB / RGBA, 16 for FXT1 -- per 8x4 texels, two source blocks
bool etc1s_transcode_is_pixel_target(uint32_t target);
// one launch; d_invalid is cleared first and afterwards holds how many blocks had an index past its palette (their output is zero-filled)
// chroma_filter: BC7 only, the reference's default
hipError_t launch_transcode_etc1s(hipStream_t st, const etc1s_transcode_args& a, uint32_t target, bool chroma_filter = false);
// one launch over every slice of the table; invalid[n_slices] is cleared first and afterwards holds the per-slice counts
hipError_t launch_transcode_etc1s_slices(hipStream_t st, const etc1s_transcode_slices_args& a, uint32_t target, bool chroma_filter = false);
// fills d_tables[2 * kBc1TableEntries] with the ETC1S -> BC1 endpoint tables (5-bit, then 6-bit)
hipError_t launch_etc1s_build_bc1_tables(hipStream_t st, uint32_t* d_tables);
// fills d_tables[kEtc1sBc7TableWords]
hipError_t launch_etc1s_build_bc7_tables(hipStream_t st, uint32_t* d_tables);
// diagnostic: the chroma filter's mode-5 encoder on n_tiles tiles of 16 RGBA pixels (64 bytes each, alpha ignored) -> n_tiles opaque 16-byte blocks
hipError_t launch_bc7_mode5_tiles(hipStream_t st, const void* d_tiles, uint32_t n_tiles, void* d_out, const uint32_t* bc7_tables);
// fills d_tables[kEtc1sAstcTableWords]
hipError_t launch_etc1s_build_astc_tables(hipStream_t st, uint32_t* d_tables);
// fills d_tables[kEtc1sAtcTableWords]
hipError_t launch_etc1s_build_atc_tables(hipStream_t st, uint32_t* d_tables);
// the launch for a target of ANY family, which every entry goes through behind its family's target check: ATC RGB, PVRTC2 RGB / RGBA (atc_tables) and FXT1
// (a.bc1_endpoints; rows of (nbx + 1) / 2 blocks) by kernels of their own, any other target as launch_transcode_etc1s / _slices. The count is of source blocks.
hipError_t launch_transcode_etc1s_any_target(hipStream_t st, const etc1s_transcode_args& a, const uint32_t* atc_tables, uint32_t target, bool chroma_filter = false);
hipError_t launch_transcode_etc1s_any_target_slices(hipStream_t st, const etc1s_transcode_slices_args& a, const uint32_t* atc_tables, uint32_t target, bool chroma_filter = false);
// counts the entries of idx[n] that are >= limit into *d_count (cleared first)
hipError_t launch_etc1s_count_indices_past(hipStream_t st, const uint16_t* idx, uint32_t n, uint32_t limit, uint32_t* d_count, bool clear);

}  // namespace bu
