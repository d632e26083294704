// Test-only C wrapper over basis_universal_amd/csrc/tile_geometry_check.h (g++, no HIP): the geometry defaults and refusals, the output-size arithmetic, the slice
// tables and the raster-pair check that the entries of the C ABI run before they touch a context, so that the CPU suite can hold their texts and their packs.
#include <string.h>
#include "../../basis_universal_amd/csrc/tile_geometry_check.h"
#include "host_api.h"

using namespace bu;

// uastc_limits != 0: transcode_uastc's limit (2^31 - 1 blocks in all) instead of 16384 each way. out6: nbx, nby, width, height, pitch, rows
HOST_API int tg_resolve(const char* who, uint32_t uastc_limits, uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t pitch, uint32_t rows, uint32_t* out6,
                        char* err, size_t err_size) {
    tile_geometry g = { 0, 0, 0, 0, 0, 0 };
    const int ok = resolve_geometry(who, nbx, nby, orig_w, orig_h, pitch, rows, uastc_limits ? kUastcOneImage : kEachWay16384, &g, err_text{ err, err_size });
    if (ok) memcpy(out6, &g, sizeof(g));
    return ok;
}

HOST_API size_t tg_output_bytes(uint32_t nbx, uint32_t nby, uint32_t orig_w, uint32_t orig_h, uint32_t pitch, uint32_t rows, uint32_t unit, uint32_t is_pixel_target) {
    return raster_output_bytes(tile_geometry{ nbx, nby, orig_w, orig_h, pitch, rows }, unit, is_pixel_target != 0);
}

// layout4: the pack's size, prefix_at, counters_at, the total of items; the pack itself is copied where it fits `capacity`
static int table_out(const slice_table& t, int ok, uint8_t* out_pack, size_t capacity, uint64_t* layout4) {
    if (!ok) return 0;
    layout4[0] = t.pack.size(); layout4[1] = t.prefix_at; layout4[2] = t.counters_at; layout4[3] = t.total;
    if (t.pack.size() > capacity || t.upload_bytes() != t.counters_at || t.prefix()[t.n] != t.total) return -1;
    memcpy(out_pack, t.pack.data(), t.pack.size());
    return 1;
}

// policy 0 / 1: the UASTC / ETC1S whole-file transcoder for a target of `unit` bytes per block or pixel; 2: the DDS pixel packer for a format of `unit` bytes per pixel
HOST_API int tg_transcode_table(uint32_t policy, const char* fn, const void* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t unit, uint32_t is_pixel_target,
                                const char* target_name, uint64_t d_out, size_t out_bytes, uint8_t* out_pack, size_t capacity, uint64_t* layout4, char* err, size_t err_size) {
    const slice_policy p = policy == 2 ? dds_pixels_slice_policy(unit) : transcoder_slice_policy(policy == 1, unit, is_pixel_target != 0, target_name);
    slice_table t;
    const int ok = build_transcode_slices(t, fn, static_cast<const bu_hip_transcode_slice*>(slices), n_slices, n_inputs, p, reinterpret_cast<const void*>((uintptr_t)d_out),
                                          out_bytes, err_text{ err, err_size });
    return table_out(t, ok, out_pack, capacity, layout4);
}

HOST_API int tg_source_table(const char* fn, const void* slices, uint32_t n, uint64_t d_out, uint8_t* out_pack, size_t capacity, uint64_t* layout4, char* err, size_t err_size) {
    slice_table t;
    const int ok = build_source_slices(t, fn, static_cast<const bu_hip_slice_source*>(slices), n, reinterpret_cast<const void*>((uintptr_t)d_out), err_text{ err, err_size });
    return table_out(t, ok, out_pack, capacity, layout4);
}

// out4: pitch a, pitch b, the region's width and height
HOST_API int tg_pair_region(const char* fn, uint64_t d_a, uint32_t wa, uint32_t ha, uint32_t pitch_a, uint64_t d_b, uint32_t wb, uint32_t hb, uint32_t pitch_b, uint32_t max_dim,
                            uint32_t* out4, char* err, size_t err_size) {
    uint32_t w = 0, h = 0;
    const int ok = raster_pair_region(fn, reinterpret_cast<const void*>((uintptr_t)d_a), wa, ha, &pitch_a, reinterpret_cast<const void*>((uintptr_t)d_b), wb, hb, &pitch_b, &w, &h,
                                      max_dim, err_text{ err, err_size });
    if (ok) { out4[0] = pitch_a; out4[1] = pitch_b; out4[2] = w; out4[3] = h; }
    return ok;
}
