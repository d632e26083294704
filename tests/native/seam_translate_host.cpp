// seam_translate_host.cpp -- test-only shim over basis_universal_amd/csrc/host/seam_translate.h (helpers.seam_translate_host()): the host translations of
// section 1 of include/basisu_hip.h, callable without a GPU. A translation returns a handle holding its tables as byte blobs (st_get copies one out), or
// NULL with *err set to the refusal's text -- the text bu_hip_last_error reports when the real entry point refuses the same input.
//   st_refine: 0 params u32 | 1 cand_offsets u32 | 2 cand_indices u32 | 3 block_parent u8 | 4 block_cur u32
//   st_fosc:   0 selector_blocks 8 B | 1 encoded_blocks 8 B | 2 cand_offsets u32 | 3 cand_indices u32 | 4 block_parent u8
//   st_pixel_clusters: 0 texels u32 | 1 offsets u32 | 2 indices u32 | 3 reps u32 | 4 totals u64
// Built and bound by tests/native_libs.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../basis_universal_amd/csrc/host/seam_translate.h"
#include "host_api.h"

namespace {
struct handle { std::vector<std::vector<uint8_t>> blobs; };
template <typename T> void add(handle* h, const std::vector<T>& v) {
    std::vector<uint8_t> b(v.size() * sizeof(T));
    if (!b.empty()) std::memcpy(b.data(), v.data(), b.size());
    h->blobs.push_back(std::move(b));
}
void add_windows(handle* h, const bu::seam::windows& w) { add(h, w.cand_offsets); add(h, w.cand_indices); add(h, w.block_parent); }
}  // namespace

HOST_API void* st_refine(const void* info, uint32_t n_blocks, uint32_t total_clusters, const void* clusters, const char** err) {
    bu::seam::refine_tables t;
    if ((*err = bu::seam::translate_refine(static_cast<const bu_block_info*>(info), n_blocks, total_clusters, static_cast<const bu_endpoint_cluster*>(clusters), t))) return nullptr;
    handle* h = new handle();
    add(h, t.params); add_windows(h, t.win); add(h, t.block_cur);
    return h;
}
HOST_API void* st_fosc(const void* info, uint32_t n_blocks, uint32_t total_selectors, const void* selectors, const char** err) {
    bu::seam::fosc_tables t;
    if ((*err = bu::seam::translate_fosc(static_cast<const bu_fosc_block*>(info), n_blocks, total_selectors, static_cast<const bu_fosc_selector*>(selectors), t))) return nullptr;
    handle* h = new handle();
    add(h, t.selector_blocks); add(h, t.encoded_blocks); add_windows(h, t.win);
    return h;
}
HOST_API void* st_pixel_clusters(uint32_t total_clusters, const void* clusters, uint64_t total_pixels, const void* pixels, const uint32_t* weights, const char** err) {
    bu::seam::pixel_tables t;
    if ((*err = bu::seam::translate_pixel_clusters(total_clusters, static_cast<const bu_pixel_cluster*>(clusters), total_pixels, static_cast<const bu_color_rgba*>(pixels), weights, t)))
        return nullptr;
    handle* h = new handle();
    add(h, t.texels); add(h, t.offsets); add(h, t.indices); add(h, t.reps); add(h, t.totals);
    return h;
}
// bytes of blob `what` (~0 for a bad index); copied to dst when cap_bytes covers them
HOST_API uint64_t st_get(void* p, uint32_t what, void* dst, uint64_t cap_bytes) {
    handle* h = static_cast<handle*>(p);
    if (!h || what >= h->blobs.size()) return ~0ull;
    const std::vector<uint8_t>& b = h->blobs[what];
    if (dst && cap_bytes >= b.size() && !b.empty()) std::memcpy(dst, b.data(), b.size());
    return b.size();
}
HOST_API void st_free(void* p) { delete static_cast<handle*>(p); }
HOST_API void st_selectors_to_etc_block(uint32_t packed, uint8_t out[8]) { const uint64_t v = bu::seam::selectors_to_etc_block(packed); std::memcpy(out, &v, 8); }
HOST_API void st_color5_inten_to_etc_block(uint32_t r5, uint32_t g5, uint32_t b5, uint32_t inten, uint8_t out[8]) {
    const uint64_t v = bu::seam::color5_inten_to_etc_block(r5, g5, b5, inten);
    std::memcpy(out, &v, 8);
}
HOST_API uint32_t st_max_windows(void) { return bu::seam::MAX_WINDOWS; }
HOST_API uint64_t st_max_expanded_texels(void) { return bu::seam::MAX_EXPANDED_TEXELS; }
