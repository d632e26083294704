// etc1s_transcode_kernels.hip -- the texel half of basisu_lowlevel_etc1s_transcoder::transcode_slice (transcoder/basisu_transcoder.cpp:8858-9345) over the indices
// host/etc1s_decode.cpp produced: one lane per 4x4 block, one launch per image, the target a template parameter so that each instance carries only its own path.
// A lane reads its two u16 indices (four with an alpha slice), gathers the palette entries (4 bytes each) and builds its output in registers: block targets store
// one uint2 per block, consecutive lanes on consecutive blocks; pixel targets store the four rows of the tile into the caller's raster, cropped to the image, as
// one 16-byte (RGBA32) or 8-byte (16-bit formats) word per row where the row is whole and aligned. An index past its palette never reaches a gather: the block is
// zero-filled and counted with a vector atomic, and it does not stop the others. Two kernels share that per-block work: one image per launch, and every image of
// a file in one launch through a slice table (tile_raster.h), counted per slice.
// The 16-byte targets (ETC2 RGBA, BC7 mode 5) store one uint4 per block; their conversions are etc1s_texture_targets.h's. BC7's chroma filter is a second template
// parameter, so the unfiltered instance carries none of the encoder. ASTC 4x4 (16 bytes), EAC R11 (8) and EAC RG11 (16) are etc1s_block_format_targets.h's.
// ATC RGB, PVRTC2 4bpp RGB (8 bytes) and FXT1 (16 bytes per 8x4 texels, two source blocks) are etc1s_vendor_format_targets.h's, behind kernels of their own.
#include <hip/hip_runtime.h>
#include "etc1s_device.h"
#include "etc1s_transcode_kernels.h"
#include "tile_raster.h"

#define BU_TAB static __device__ const
#include "etc1s_transcode_tables.inc"
#include "uastc_transcode_tables.inc"   // ku_trit_encode, for ASTC's endpoints of range 0..47
#undef BU_TAB

namespace bu {

struct etc1s_entry { uint32_t r5, g5, b5, table; };
__device__ __forceinline__ etc1s_entry unpack_entry(uint32_t e) { return etc1s_entry{ e & 31u, (e >> 8) & 31u, (e >> 16) & 31u, (e >> 24) & 7u }; }
__device__ __forceinline__ uint32_t texel_selector(uint32_t sel, uint32_t x, uint32_t y) { return (sel >> (2u * (y * 4u + x))) & 3u; }

// the four colours of an entry, r | g << 8 | b << 16 (get_block_colors5, transcoder.cpp:996-1010)
__device__ __forceinline__ void block_colors(const etc1s_entry& e, uint32_t out[4]) {
    const int r = scale5((int)e.r5), g = scale5((int)e.g5), b = scale5((int)e.b5);
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int d = inten_delta((int)e.table, s);
        out[s] = (uint32_t)clamp255(r + d) | ((uint32_t)clamp255(g + d) << 8) | ((uint32_t)clamp255(b + d) << 16);
    }
}
__device__ __forceinline__ uint32_t pick4(const uint32_t c[4], uint32_t s) {   // c[s] as selects: a dynamic index would put the array in scratch memory
    const uint32_t lo = (s & 1u) ? c[1] : c[0], hi = (s & 1u) ? c[3] : c[2];
    return (s & 2u) ? hi : lo;
}

// cETC1 (transcoder.cpp:8863-8875): a differential block whose two halves have the same colour and table, delta 0, flip bit clear; the block's 64 bits as the big-endian
// value V (etc1s_device.h), returned as it lies in memory
__device__ __forceinline__ uint2 to_etc1(const etc1s_entry& e, uint32_t sel) {
    const uint32_t hi = (e.r5 << 27) | (e.g5 << 19) | (e.b5 << 11) | (e.table << 5) | (e.table << 2) | 2u;
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t y = 0; y < 4; y++)
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) lo |= selector_bits(x, y, texel_selector(sel, x, y));
    return make_uint2(__builtin_bswap32(hi), __builtin_bswap32(lo));
}

}  // namespace bu
#include "etc1s_bc1.h"
#include "etc1s_texture_targets.h"
#include "etc1s_block_format_targets.h"
#include "etc1s_vendor_format_targets.h"
namespace bu {
static_assert(kBc7TableWords == kEtc1sBc7TableWords, "the header's size of the BC7 tables");
static_assert(kAstcTableWords == kEtc1sAstcTableWords, "the header's size of the ASTC tables");
static_assert(kAtcTableWords == kEtc1sAtcTableWords, "the header's size of the ATC tables");

// one pixel of a pixel target from the block colour (r | g << 8 | b << 16) and the alpha value (transcoder.cpp:9155-9332; the 4444 colour pass ORs onto the alpha pass)
template <uint32_t TARGET>
__device__ __forceinline__ uint32_t pack_pixel(uint32_t c, uint32_t a) {
    const uint32_t r = c & 255u, g = (c >> 8) & 255u, b = c >> 16;
    if (TARGET == ETF_RGBA32) return c | (a << 24);
    if (TARGET == ETF_RGB565) return pack_rgb565(r, g, b);   // mul_8 and the packs: tile_raster.h, shared with the UASTC transcoder
    if (TARGET == ETF_BGR565) return pack_rgb565(b, g, r);
    return pack_rgba4444(r, g, b, a);
}

// what every block of a launch reads besides its own indices
struct etc1s_palettes {
    const uint32_t *endpoint_palette, *selector_palette, *bc1_endpoints, *bc7_tables, *astc_tables;
    uint32_t n_endpoints, n_selectors;
};

// One block: the range check, the gathers, the target's conversion, the store. The four index pointers are the IMAGE's (alpha: both null = opaque), `out` is where
// the image's output begins, `i` the block's place in the image's raster order. Block targets write one uint2 at out[i]; pixel targets the four rows of the tile
// cropped to width x min(height, rows) (store_tile_row, tile_raster.h). false = an index was past its palette and zeros were written.
// Both kernels below are this function behind their own indexing. FILTER: BC7's chroma filter.
template <uint32_t TARGET, bool FILTER>
__device__ __forceinline__ bool transcode_etc1s_block(const etc1s_palettes& a, const uint16_t* endpoint_idx, const uint16_t* selector_idx, const uint16_t* alpha_endpoint_idx,
                                                      const uint16_t* alpha_selector_idx, void* out, uint32_t i, const tile_geometry& g) {
    constexpr bool kPixels = TARGET == ETF_RGBA32 || TARGET == ETF_RGB565 || TARGET == ETF_BGR565 || TARGET == ETF_RGBA4444;
    constexpr bool kWide = TARGET == ETF_ETC2_RGBA || TARGET == ETF_BC7_RGBA || TARGET == ETF_ASTC_4x4_RGBA || TARGET == ETF_ETC2_EAC_RG11;   // 16 bytes per block, both slices
    constexpr bool kAlpha = TARGET == ETF_RGBA32 || TARGET == ETF_RGBA4444 || kWide;
    const uint32_t ei = endpoint_idx[i], si = selector_idx[i];
    bool ok = ei < a.n_endpoints && si < a.n_selectors;
    uint32_t aei = 0, asi = 0;
    const bool has_alpha = kAlpha && alpha_endpoint_idx != nullptr;
    if (has_alpha) {
        aei = alpha_endpoint_idx[i]; asi = alpha_selector_idx[i];
        ok = ok && aei < a.n_endpoints && asi < a.n_selectors;
    }
    if (kWide) {
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (ok) {
            const uint32_t entry = a.endpoint_palette[ei], sel = a.selector_palette[si];
            const etc1s_entry e = unpack_entry(entry);
            if (TARGET == ETF_ETC2_RGBA) {
                const uint2 alpha = has_alpha ? to_eac_a8(unpack_entry(a.endpoint_palette[aei]), a.selector_palette[asi]) : opaque_eac_a8(), rgb = to_etc1(e, sel);
                o = make_uint4(alpha.x, alpha.y, rgb.x, rgb.y);
            } else if (TARGET == ETF_ETC2_EAC_RG11) {
                const uint2 red = to_eac_r11(e, sel), green = has_alpha ? to_eac_r11(unpack_entry(a.endpoint_palette[aei]), a.selector_palette[asi]) : opaque_eac_a8();
                o = make_uint4(red.x, red.y, green.x, green.y);
            } else if (TARGET == ETF_ASTC_4x4_RGBA) {
                const astc_block b = to_astc(e, sel, has_alpha, has_alpha ? unpack_entry(a.endpoint_palette[aei]) : e, has_alpha ? a.selector_palette[asi] : 0u, a.astc_tables);
                o = make_uint4((uint32_t)b.lo, (uint32_t)(b.lo >> 32), (uint32_t)b.hi, (uint32_t)(b.hi >> 32));
            } else {
                bc7_m5 b = to_bc7_m5_color(e, sel, a.bc7_tables);
                if (FILTER)
                    b = bc7_chroma_filter(b, a.endpoint_palette, a.n_endpoints, endpoint_idx, entry, i % g.nbx, i / g.nbx, g.nbx, g.nby,
                                          reinterpret_cast<const float*>(a.bc7_tables + kBc7ColorEntries));
                if (has_alpha) bc7_m5_alpha(b, unpack_entry(a.endpoint_palette[aei]), a.selector_palette[asi]);
                o = make_uint4((uint32_t)b.lo, (uint32_t)(b.lo >> 32), (uint32_t)b.hi, (uint32_t)(b.hi >> 32));
            }
        }
        ((uint4*)out)[i] = o;
        return ok;
    }
    if (!kPixels) {
        uint2 o = make_uint2(0u, 0u);
        if (ok) {
            const etc1s_entry e = unpack_entry(a.endpoint_palette[ei]);
            const uint32_t sel = a.selector_palette[si];
            o = TARGET == ETF_ETC1_RGB ? to_etc1(e, sel) : (TARGET == ETF_ETC2_EAC_R11 ? to_eac_r11(e, sel) : to_bc1<true>(e, sel, a.bc1_endpoints, a.bc1_endpoints + kBc1TableEntries));
        }
        ((uint2*)out)[i] = o;
        return ok;
    }
    uint32_t colors[4] = { 0, 0, 0, 0 }, alphas[4] = { 255u, 255u, 255u, 255u }, sel = 0, asel = 0;
    if (ok) {
        block_colors(unpack_entry(a.endpoint_palette[ei]), colors);
        sel = a.selector_palette[si];
        if (has_alpha) {   // alpha = the green channel of the alpha slice's block colours
            uint32_t ac[4];
            block_colors(unpack_entry(a.endpoint_palette[aei]), ac);
#pragma unroll
            for (int s = 0; s < 4; s++) alphas[s] = (ac[s] >> 8) & 255u;
            asel = a.selector_palette[asi];
        }
    } else {
        alphas[0] = alphas[1] = alphas[2] = alphas[3] = 0;
    }
    constexpr uint32_t kUnit = TARGET == ETF_RGBA32 ? 4u : 2u;
    const uint32_t bx = i % g.nbx, by = i / g.nbx;
#pragma unroll
    for (uint32_t y = 0; y < 4; y++) {
        const uint32_t row = by * 4u + y;
        if (row >= g.height || row >= g.rows) break;
        uint32_t v[4];
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) {
            const uint32_t px = pack_pixel<TARGET>(pick4(colors, texel_selector(sel, x, y)), has_alpha ? pick4(alphas, texel_selector(asel, x, y)) : alphas[0]);
            v[x] = ok ? px : 0u;
        }
        store_tile_row(kUnit, (uint8_t*)out + ((size_t)row * g.pitch + bx * 4u) * kUnit, bx, g.width, v);
    }
    return ok;
}

template <uint32_t TARGET, bool FILTER>
__global__ __launch_bounds__(256) void transcode_etc1s_kernel(etc1s_transcode_args a) {
    const uint32_t n = a.g.nbx * a.g.nby, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const etc1s_palettes p = { a.endpoint_palette, a.selector_palette, a.bc1_endpoints, a.bc7_tables, a.astc_tables, a.n_endpoints, a.n_selectors };
    if (!transcode_etc1s_block<TARGET, FILTER>(p, a.endpoint_idx, a.selector_idx, a.alpha_endpoint_idx, a.alpha_selector_idx, a.out, i, a.g)) atomicAdd(a.invalid, 1u);
}

// every image of a file in one launch (bu_hip_k_transcode_etc1s_slices): find_transcode_slice (tile_raster.h) in front of the same block function. The colour and the
// alpha slice of an image are two ranges of the same two index arrays.
template <uint32_t TARGET, bool FILTER>
__global__ __launch_bounds__(256) void transcode_etc1s_slices_kernel(etc1s_transcode_slices_args a) {
    transcode_slice_view v;
    if (!find_transcode_slice(a.slices, a.prefix, a.n_slices, a.total_blocks, blockIdx.x * 256u + threadIdx.x, v)) return;
    const etc1s_palettes p = { a.endpoint_palette, a.selector_palette, a.bc1_endpoints, a.bc7_tables, a.astc_tables, a.n_endpoints, a.n_selectors };
    const bool alpha = v.alpha_first_block != BU_HIP_NO_ALPHA_SLICE;
    if (!transcode_etc1s_block<TARGET, FILTER>(p, a.endpoint_idx + v.first_block, a.selector_idx + v.first_block, alpha ? a.endpoint_idx + v.alpha_first_block : nullptr,
                                               alpha ? a.selector_idx + v.alpha_first_block : nullptr, a.out + v.out_offset, v.local, v.g))
        atomicAdd(a.invalid + v.slice, 1u);
}

// The two endpoint tables of to_bc1, [intensity table][base5][range][mapping] -> lo | hi << 8 | squared error << 16 for 5-bit (first kBc1TableEntries words) and 6-bit
// endpoints: one lane per entry searches every endpoint pair, hi outermost, lo innermost, first minimum (tools/gen_etc1s_transcode_tables.py's endpoint_table() is the
// same search on the host). 30,720 lanes x at most 4,096 pairs x at most 4 selectors: well under a millisecond, once per context.
__global__ __launch_bounds__(256) void etc1s_build_bc1_tables_kernel(uint32_t* tables) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= 2u * kBc1TableEntries) return;
    const bool six = idx >= kBc1TableEntries;
    const uint32_t e = six ? idx - kBc1TableEntries : idx, m = e % 10u, r = (e / 10u) % 6u, g = (e / 60u) % 32u, t = e / 1920u;
    const int base = scale5((int)g);
    int block[4];
#pragma unroll
    for (int s = 0; s < 4; s++) block[s] = clamp255(base + inten_delta((int)t, s));
    const uint32_t s0 = ke_bc1_ranges[r * 2], s1 = ke_bc1_ranges[r * 2 + 1];
    const uint32_t m0 = ke_bc1_mappings[m * 4], m1 = ke_bc1_mappings[m * 4 + 1], m2 = ke_bc1_mappings[m * 4 + 2], m3 = ke_bc1_mappings[m * 4 + 3];
    const uint32_t n = six ? 64u : 32u;
    uint32_t best_err = 0xFFFFFFFFu, best_lo = 0, best_hi = 0;
    for (uint32_t hi = 0; hi < n; hi++)
        for (uint32_t lo = 0; lo < n; lo++) {
            uint32_t c[4];
            c[0] = six ? ((lo << 2) | (lo >> 4)) : ((lo << 3) | (lo >> 2));
            c[3] = six ? ((hi << 2) | (hi >> 4)) : ((hi << 3) | (hi >> 2));
            c[1] = (c[0] * 2u + c[3]) / 3u;
            c[2] = (c[3] * 2u + c[0]) / 3u;
            const uint32_t mapped[4] = { pick4(c, m0), pick4(c, m1), pick4(c, m2), pick4(c, m3) };
            uint32_t err = 0;
#pragma unroll
            for (uint32_t s = 0; s < 4; s++) {
                const int d = block[s] - (int)mapped[s];
                if (s >= s0 && s <= s1) err += (uint32_t)(d * d);
            }
            if (err < best_err) { best_err = err; best_lo = lo; best_hi = hi; }
        }
    tables[idx] = best_lo | (best_hi << 8) | (best_err << 16);
}

// The colour look-up of to_bc7_m5_color, [intensity table][base5][range][mapping] -> lo | hi << 8 | min(error, 65535) << 16 over 7-bit endpoints, and behind it the
// encoder's 128 midpoints. The search is the BC1 tables' (hi outermost, lo innermost, first minimum; bc7_color_table() of the tool on the host), over BC7's four
// colours (weights 0, 21, 43, 64 of 64, rounded), and with the errors of selectors 0 and 3 counted five times for the widest intensity table over the whole range.
__global__ __launch_bounds__(256) void etc1s_build_bc7_tables_kernel(uint32_t* tables) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kBc7TableWords) return;
    if (idx >= kBc7ColorEntries) { tables[idx] = __float_as_uint(mode5_midpoint(idx - kBc7ColorEntries)); return; }
    const uint32_t m = idx % 10u, r = (idx / 10u) % 6u, g = (idx / 60u) % 32u, t = idx / 1920u;
    const int base = scale5((int)g);
    int block[4];
#pragma unroll
    for (int s = 0; s < 4; s++) block[s] = clamp255(base + inten_delta((int)t, s));
    const uint32_t s0 = ke_bc1_ranges[r * 2], s1 = ke_bc1_ranges[r * 2 + 1];
    const uint32_t m0 = ke_bc1_mappings[m * 4], m1 = ke_bc1_mappings[m * 4 + 1], m2 = ke_bc1_mappings[m * 4 + 2], m3 = ke_bc1_mappings[m * 4 + 3];
    const uint32_t ends_weight = (t == 7u && s0 == 0u && s1 == 3u) ? 5u : 1u;
    uint32_t best_err = 0xFFFFFFFFu, best_lo = 0, best_hi = 0;
    for (uint32_t hi = 0; hi < 128u; hi++)
        for (uint32_t lo = 0; lo < 128u; lo++) {
            uint32_t c[4];
            c[0] = from_7(lo);
            c[3] = from_7(hi);
            c[1] = (c[0] * 43u + c[3] * 21u + 32u) / 64u;
            c[2] = (c[0] * 21u + c[3] * 43u + 32u) / 64u;
            const uint32_t mapped[4] = { pick4(c, m0), pick4(c, m1), pick4(c, m2), pick4(c, m3) };
            uint32_t err = 0;
#pragma unroll
            for (uint32_t s = 0; s < 4; s++) {
                const int d = block[s] - (int)mapped[s];
                if (s >= s0 && s <= s1) err += (uint32_t)(d * d) * ((s == 0u || s == 3u) ? ends_weight : 1u);
            }
            if (err < best_err) { best_err = err; best_lo = lo; best_hi = hi; }
        }
    tables[idx] = best_lo | (best_hi << 8) | ((best_err < 0xFFFFu ? best_err : 0xFFFFu) << 16);
}

// The two look-ups of to_astc, [intensity table][base5][range][mapping] -> lo | hi << 8 | error << 16: over the 48 BISE codes of endpoint range 0..47 in code order
// (first kAstcEntries words), then over 8-bit endpoints; behind them the 48 unquantised values. The search is the BC7 table's (hi outermost, lo innermost, first
// minimum) over ASTC's four values, the errors of selectors 0 and 3 counted eight times for the widest intensity table over the whole range. The ten errors of an
// entry are stored as they are while the largest fits 16 bits; else each times 65535 over that largest, rounded to nearest. A workgroup is 25 entries of ten lanes,
// so that the ten meet in LDS. astc_table_0_47() / astc_table_0_255() of the tool are the same on the host.
__global__ __launch_bounds__(256) void etc1s_build_astc_tables_kernel(uint32_t* tables) {
    __shared__ uint32_t raw[250];
    const uint32_t idx = blockIdx.x * 250u + threadIdx.x;
    const bool lane = threadIdx.x < 250u && idx < 2u * kAstcEntries;
    if (blockIdx.x == 0 && threadIdx.x >= 250u) {   // the six idle lanes of the first workgroup write the unquantised values
        for (uint32_t c = threadIdx.x - 250u; c < 48u; c += 6u) tables[2u * kAstcEntries + c] = astc_unquant48(c);
    }
    uint32_t best_err = 0xFFFFFFFFu, best_lo = 0, best_hi = 0;
    if (lane) {
        const bool wide = idx >= kAstcEntries;
        const uint32_t e = wide ? idx - kAstcEntries : idx, m = e % 10u, r = (e / 10u) % 6u, g = (e / 60u) % 32u, t = e / 1920u;
        const int base = scale5((int)g);
        int block[4];
#pragma unroll
        for (int s = 0; s < 4; s++) block[s] = clamp255(base + inten_delta((int)t, s));
        const uint32_t s0 = ke_bc1_ranges[r * 2], s1 = ke_bc1_ranges[r * 2 + 1];
        const uint32_t m0 = ke_bc1_mappings[m * 4], m1 = ke_bc1_mappings[m * 4 + 1], m2 = ke_bc1_mappings[m * 4 + 2], m3 = ke_bc1_mappings[m * 4 + 3];
        const uint32_t ends_weight = (t == 7u && s0 == 0u && s1 == 3u) ? 8u : 1u;
        const uint32_t n = wide ? 256u : 48u;
        for (uint32_t hi = 0; hi < n; hi++) {
            const uint32_t vh = wide ? hi : astc_unquant48(hi);
            for (uint32_t lo = 0; lo < n; lo++) {
                const uint32_t vl = wide ? lo : astc_unquant48(lo);
                const uint32_t c[4] = { astc_interp2(vl, vh, 0u), astc_interp2(vl, vh, 21u), astc_interp2(vl, vh, 43u), astc_interp2(vl, vh, 64u) };
                const uint32_t mapped[4] = { pick4(c, m0), pick4(c, m1), pick4(c, m2), pick4(c, m3) };
                uint32_t err = 0;
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) {
                    const int d = block[s] - (int)mapped[s];
                    if (s >= s0 && s <= s1) err += (uint32_t)(d * d) * ((s == 0u || s == 3u) ? ends_weight : 1u);
                }
                if (err < best_err) { best_err = err; best_lo = lo; best_hi = hi; }
            }
        }
        raw[threadIdx.x] = best_err;
    }
    __syncthreads();
    if (!lane) return;
    const uint32_t first = threadIdx.x - threadIdx.x % 10u;
    uint32_t top = 0;
    for (uint32_t k = 0; k < 10u; k++) top = raw[first + k] > top ? raw[first + k] : top;
    if (top > 0xFFFFu) best_err = (uint32_t)((2ull * best_err * 0xFFFFull + top) / (2ull * top));
    tables[idx] = best_lo | (best_hi << 8) | (best_err << 16);
}

// ---- the fourth family's own targets: vendor_format_block (etc1s_vendor_format_targets.h) behind the two kinds of indexing. FXT1 runs a lane per SOURCE block like the
// others, so that the slice table's block counts hold for it too; the lanes of odd block columns have nothing to do.
static_assert(VF_ATC_RGB == ETF_ATC_RGB && VF_FXT1_RGB == ETF_FXT1_RGB && VF_PVRTC2_4_RGB == ETF_PVRTC2_4_RGB && VF_PVRTC2_4_RGBA == ETF_PVRTC2_4_RGBA,
              "the header's target numbers");
template <uint32_t TARGET>
__global__ __launch_bounds__(256) void transcode_etc1s_vendor_kernel(etc1s_transcode_args a, const uint32_t* atc_tables) {
    const uint32_t n = a.g.nbx * a.g.nby, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const vendor_format_inputs p = { a.endpoint_palette, a.selector_palette, a.bc1_endpoints, a.bc1_endpoints + kBc1TableEntries, atc_tables, a.n_endpoints, a.n_selectors };
    const uint32_t bad = vendor_format_block<TARGET>(p, a.endpoint_idx, a.selector_idx, a.alpha_endpoint_idx, a.alpha_selector_idx, a.out, i, a.g.nbx);
    if (bad) atomicAdd(a.invalid, bad);
}

template <uint32_t TARGET>
__global__ __launch_bounds__(256) void transcode_etc1s_vendor_slices_kernel(etc1s_transcode_slices_args a, const uint32_t* atc_tables) {
    transcode_slice_view v;
    if (!find_transcode_slice(a.slices, a.prefix, a.n_slices, a.total_blocks, blockIdx.x * 256u + threadIdx.x, v)) return;
    const vendor_format_inputs p = { a.endpoint_palette, a.selector_palette, a.bc1_endpoints, a.bc1_endpoints + kBc1TableEntries, atc_tables, a.n_endpoints, a.n_selectors };
    const bool alpha = v.alpha_first_block != BU_HIP_NO_ALPHA_SLICE;
    const uint32_t bad = vendor_format_block<TARGET>(p, a.endpoint_idx + v.first_block, a.selector_idx + v.first_block, alpha ? a.endpoint_idx + v.alpha_first_block : nullptr,
                                                     alpha ? a.selector_idx + v.alpha_first_block : nullptr, a.out + v.out_offset, v.local, v.g.nbx);
    if (bad) atomicAdd(a.invalid + v.slice, bad);
}

// The three look-ups of atc_solve, [intensity table][base5][range][mapping] -> lo | hi << 8 | min(error, 65535) << 16: "55" (both endpoints 5 bits), "56" (a 6-bit high
// endpoint) and "45" (PVRTC2's 4-bit low endpoint, expanded to 5 bits and then to 8), kAtcEntries words each. One lane per entry. The search is the BC7 table's (hi
// outermost, lo innermost, first minimum; the errors of selectors 0 and 3 counted five times for the widest intensity table over the whole range) over the values
// lo, (5 lo + 3 hi) / 8, (3 lo + 5 hi) / 8, hi. atc_endpoint_table() of the tool is the same search on the host.
__global__ __launch_bounds__(256) void etc1s_build_atc_tables_kernel(uint32_t* tables) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kAtcTableWords) return;
    const uint32_t which = idx / kAtcEntries, e = idx % kAtcEntries, m = e % 10u, r = (e / 10u) % 6u, g = (e / 60u) % 32u, t = e / 1920u;
    const int base = scale5((int)g);
    int block[4];
#pragma unroll
    for (int s = 0; s < 4; s++) block[s] = clamp255(base + inten_delta((int)t, s));
    const uint32_t s0 = ke_bc1_ranges[r * 2], s1 = ke_bc1_ranges[r * 2 + 1];
    const uint32_t m0 = ke_bc1_mappings[m * 4], m1 = ke_bc1_mappings[m * 4 + 1], m2 = ke_bc1_mappings[m * 4 + 2], m3 = ke_bc1_mappings[m * 4 + 3];
    const uint32_t ends_weight = (t == 7u && s0 == 0u && s1 == 3u) ? 5u : 1u;
    const uint32_t n_lo = which == 2u ? 16u : 32u, n_hi = which == 1u ? 64u : 32u;
    uint32_t best_err = 0xFFFFFFFFu, best_lo = 0, best_hi = 0;
    for (uint32_t hi = 0; hi < n_hi; hi++)
        for (uint32_t lo = 0; lo < n_lo; lo++) {
            const uint32_t lo5 = which == 2u ? ((lo << 1) | (lo >> 3)) : lo;
            uint32_t c[4];
            c[0] = (lo5 << 3) | (lo5 >> 2);
            c[3] = which == 1u ? ((hi << 2) | (hi >> 4)) : ((hi << 3) | (hi >> 2));
            c[1] = (c[0] * 5u + c[3] * 3u) / 8u;
            c[2] = (c[3] * 5u + c[0] * 3u) / 8u;
            const uint32_t mapped[4] = { pick4(c, m0), pick4(c, m1), pick4(c, m2), pick4(c, m3) };
            uint32_t err = 0;
#pragma unroll
            for (uint32_t s = 0; s < 4; s++) {
                const int d = block[s] - (int)mapped[s];
                if (s >= s0 && s <= s1) err += (uint32_t)(d * d) * ((s == 0u || s == 3u) ? ends_weight : 1u);
            }
            if (err < best_err) { best_err = err; best_lo = lo; best_hi = hi; }
        }
    tables[idx] = best_lo | (best_hi << 8) | ((best_err < 0xFFFFu ? best_err : 0xFFFFu) << 16);
}

__global__ __launch_bounds__(256) void etc1s_count_indices_past_kernel(const uint16_t* idx, uint32_t n, uint32_t limit, uint32_t* count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && idx[i] >= limit) atomicAdd(count, 1u);
}

// A diagnostic (bu_hip_k_bc7_mode5_tiles): the filter's encoder on tiles of the caller's choosing, one lane per tile of 16 RGBA pixels, alpha ignored.
__global__ __launch_bounds__(256) void bc7_mode5_tiles_kernel(const uint4* tiles, uint32_t n_tiles, uint4* out, const uint32_t* bc7_tables) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_tiles) return;
    uint32_t px[16];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint4 v = tiles[(size_t)i * 4u + q];
        px[q * 4u] = v.x & 0xFFFFFFu; px[q * 4u + 1u] = v.y & 0xFFFFFFu; px[q * 4u + 2u] = v.z & 0xFFFFFFu; px[q * 4u + 3u] = v.w & 0xFFFFFFu;
    }
    const bc7_m5 b = encode_bc7_mode5(px, reinterpret_cast<const float*>(bc7_tables + kBc7ColorEntries));
    out[i] = make_uint4((uint32_t)b.lo, (uint32_t)(b.lo >> 32), (uint32_t)b.hi, (uint32_t)(b.hi >> 32));
}

template <uint32_t TARGET, bool FILTER = false>
static hipError_t launch(hipStream_t st, const etc1s_transcode_args& a) {
    const uint32_t n = a.g.nbx * a.g.nby;
    hipLaunchKernelGGL((transcode_etc1s_kernel<TARGET, FILTER>), dim3((n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
template <uint32_t TARGET, bool FILTER = false>
static hipError_t launch(hipStream_t st, const etc1s_transcode_slices_args& a) {
    hipLaunchKernelGGL((transcode_etc1s_slices_kernel<TARGET, FILTER>), dim3((a.total_blocks + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// the instance of either kernel for the target
template <class Args>
static hipError_t launch_for_target(hipStream_t st, const Args& a, uint32_t target, bool chroma_filter) {
    if (target == ETF_BC1_RGB && !a.bc1_endpoints) return hipErrorInvalidValue;
    if (target == ETF_BC7_RGBA && !a.bc7_tables) return hipErrorInvalidValue;
    if (target == ETF_ASTC_4x4_RGBA && !a.astc_tables) return hipErrorInvalidValue;
    switch (target) {
    case ETF_ASTC_4x4_RGBA: return launch<ETF_ASTC_4x4_RGBA>(st, a);
    case ETF_ETC2_EAC_R11: return launch<ETF_ETC2_EAC_R11>(st, a);
    case ETF_ETC2_EAC_RG11: return launch<ETF_ETC2_EAC_RG11>(st, a);
    case ETF_ETC2_RGBA: return launch<ETF_ETC2_RGBA>(st, a);
    case ETF_BC7_RGBA: return chroma_filter ? launch<ETF_BC7_RGBA, true>(st, a) : launch<ETF_BC7_RGBA, false>(st, a);
    case ETF_ETC1_RGB: return launch<ETF_ETC1_RGB>(st, a);
    case ETF_BC1_RGB: return launch<ETF_BC1_RGB>(st, a);
    case ETF_RGBA32: return launch<ETF_RGBA32>(st, a);
    case ETF_RGB565: return launch<ETF_RGB565>(st, a);
    case ETF_BGR565: return launch<ETF_BGR565>(st, a);
    case ETF_RGBA4444: return launch<ETF_RGBA4444>(st, a);
    default: return hipErrorInvalidValue;
    }
}

template <uint32_t TARGET>
static hipError_t launch_vendor(hipStream_t st, const etc1s_transcode_args& a, const uint32_t* atc_tables) {
    const uint32_t n = a.g.nbx * a.g.nby;
    hipLaunchKernelGGL((transcode_etc1s_vendor_kernel<TARGET>), dim3((n + 255) / 256), dim3(256), 0, st, a, atc_tables);
    return hipGetLastError();
}
template <uint32_t TARGET>
static hipError_t launch_vendor(hipStream_t st, const etc1s_transcode_slices_args& a, const uint32_t* atc_tables) {
    hipLaunchKernelGGL((transcode_etc1s_vendor_slices_kernel<TARGET>), dim3((a.total_blocks + 255) / 256), dim3(256), 0, st, a, atc_tables);
    return hipGetLastError();
}
// any ETC1S target: the fourth family's own four here, any other through launch_for_target
template <class Args>
static hipError_t launch_for_any_target(hipStream_t st, const Args& a, const uint32_t* atc_tables, uint32_t target, bool chroma_filter) {
    if ((target == ETF_ATC_RGB || target == ETF_PVRTC2_4_RGB || target == ETF_PVRTC2_4_RGBA) && !atc_tables) return hipErrorInvalidValue;
    if (target == ETF_FXT1_RGB && !a.bc1_endpoints) return hipErrorInvalidValue;
    switch (target) {
    case ETF_ATC_RGB: return launch_vendor<ETF_ATC_RGB>(st, a, atc_tables);
    case ETF_FXT1_RGB: return launch_vendor<ETF_FXT1_RGB>(st, a, atc_tables);
    case ETF_PVRTC2_4_RGB: return launch_vendor<ETF_PVRTC2_4_RGB>(st, a, atc_tables);
    case ETF_PVRTC2_4_RGBA: return launch_vendor<ETF_PVRTC2_4_RGBA>(st, a, atc_tables);
    default: return launch_for_target(st, a, target, chroma_filter);
    }
}

uint32_t etc1s_transcode_unit_bytes(uint32_t target) {
    switch (target) {
    case ETF_ETC1_RGB: case ETF_BC1_RGB: return 8;
    case ETF_RGBA32: return 4;
    case ETF_RGB565: case ETF_BGR565: case ETF_RGBA4444: return 2;
    default: return 0;
    }
}
uint32_t etc1s_texture_unit_bytes(uint32_t target) { return target == ETF_ETC2_RGBA || target == ETF_BC7_RGBA ? 16u : etc1s_transcode_unit_bytes(target); }
uint32_t etc1s_block_format_unit_bytes(uint32_t target) {
    if (target == ETF_ASTC_4x4_RGBA || target == ETF_ETC2_EAC_RG11) return 16u;
    return target == ETF_ETC2_EAC_R11 ? 8u : etc1s_texture_unit_bytes(target);
}
uint32_t etc1s_vendor_format_unit_bytes(uint32_t target) {
    if (target == ETF_FXT1_RGB) return 16u;
    return target == ETF_ATC_RGB || target == ETF_PVRTC2_4_RGB || target == ETF_PVRTC2_4_RGBA ? 8u : etc1s_block_format_unit_bytes(target);
}
bool etc1s_transcode_is_pixel_target(uint32_t target) { return target == ETF_RGBA32 || target == ETF_RGB565 || target == ETF_BGR565 || target == ETF_RGBA4444; }

hipError_t launch_transcode_etc1s(hipStream_t st, const etc1s_transcode_args& a, uint32_t target, bool chroma_filter) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !a.g.nbx || !a.g.nby) return e;
    return launch_for_target(st, a, target, chroma_filter);
}

hipError_t launch_transcode_etc1s_slices(hipStream_t st, const etc1s_transcode_slices_args& a, uint32_t target, bool chroma_filter) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, (size_t)a.n_slices * sizeof(uint32_t), st);
    if (e != hipSuccess || !a.n_slices || !a.total_blocks) return e;
    return launch_for_target(st, a, target, chroma_filter);
}

hipError_t launch_etc1s_build_bc1_tables(hipStream_t st, uint32_t* d_tables) {
    hipLaunchKernelGGL(etc1s_build_bc1_tables_kernel, dim3((2u * kBc1TableEntries + 255) / 256), dim3(256), 0, st, d_tables);
    return hipGetLastError();
}

hipError_t launch_etc1s_build_bc7_tables(hipStream_t st, uint32_t* d_tables) {
    hipLaunchKernelGGL(etc1s_build_bc7_tables_kernel, dim3((kBc7TableWords + 255) / 256), dim3(256), 0, st, d_tables);
    return hipGetLastError();
}

hipError_t launch_bc7_mode5_tiles(hipStream_t st, const void* d_tiles, uint32_t n_tiles, void* d_out, const uint32_t* bc7_tables) {
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL(bc7_mode5_tiles_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, st, static_cast<const uint4*>(d_tiles), n_tiles, static_cast<uint4*>(d_out), bc7_tables);
    return hipGetLastError();
}

hipError_t launch_etc1s_build_astc_tables(hipStream_t st, uint32_t* d_tables) {
    hipLaunchKernelGGL(etc1s_build_astc_tables_kernel, dim3((2u * kAstcEntries + 249) / 250), dim3(256), 0, st, d_tables);
    return hipGetLastError();
}

hipError_t launch_transcode_etc1s_any_target(hipStream_t st, const etc1s_transcode_args& a, const uint32_t* atc_tables, uint32_t target, bool chroma_filter) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || !a.g.nbx || !a.g.nby) return e;
    return launch_for_any_target(st, a, atc_tables, target, chroma_filter);
}

hipError_t launch_transcode_etc1s_any_target_slices(hipStream_t st, const etc1s_transcode_slices_args& a, const uint32_t* atc_tables, uint32_t target, bool chroma_filter) {
    hipError_t e = hipMemsetAsync(a.invalid, 0, (size_t)a.n_slices * sizeof(uint32_t), st);
    if (e != hipSuccess || !a.n_slices || !a.total_blocks) return e;
    return launch_for_any_target(st, a, atc_tables, target, chroma_filter);
}

hipError_t launch_etc1s_build_atc_tables(hipStream_t st, uint32_t* d_tables) {
    hipLaunchKernelGGL(etc1s_build_atc_tables_kernel, dim3((kAtcTableWords + 255) / 256), dim3(256), 0, st, d_tables);
    return hipGetLastError();
}

hipError_t launch_etc1s_count_indices_past(hipStream_t st, const uint16_t* idx, uint32_t n, uint32_t limit, uint32_t* d_count, bool clear) {
    if (clear) { hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), st); if (e != hipSuccess) return e; }
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(etc1s_count_indices_past_kernel, dim3((n + 255) / 256), dim3(256), 0, st, idx, n, limit, d_count);
    return hipGetLastError();
}

}  // namespace bu
