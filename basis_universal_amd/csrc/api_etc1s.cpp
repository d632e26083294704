// api_etc1s.cpp -- ETC1S behind the C ABI of libbasisu_hip.so: resident tiles, the device-resident layer (section 2 of basisu_hip.h) and the blocking one over it (section 1).
#include <atomic>
#include <cstdlib>
#include "api_internal.h"
#include "etc1s_kernels.h"
#include "mipmap_kernels.h"
#include "unique_kernels.h"
#include "bookkeeping_kernels.h"
#include "kmeans_kernels.h"
#include "host/seam_translate.h"

namespace {
constexpr uint32_t UP_PIECE_BLOCKS = 65536;   // 4 MiB of tiles: 0.08 ms on the link, 0.11 ms of the kernel
constexpr uint32_t UP_SLOTS = 8, UP_EVENTS = 64;
unsigned upload_threads() {
    static const unsigned t = [] {
        unsigned want = 4;
        if (const char* e = std::getenv("BU_UPLOAD_THREADS")) { const int v = std::atoi(e); if (v >= 1 && v <= 16) want = (unsigned)v; }
        const unsigned hw = std::thread::hardware_concurrency();
        return hw ? std::min(want, std::max(1u, hw / 2)) : 1u;
    }();
    return t;
}
// The de-duplication and block-ranking sorts hand their item count to hipCUB as an int and size their grids in 32 bits: more than 2^30 items is refused by name, before
// any workspace is reserved and before any output is touched.
bool sort_size_ok(bu_hip_context* ctx, const char* fn, uint32_t n) {
    if (n <= (1u << 30)) return true;
    set_error(ctx, "%s: %u blocks: more than 2^30 in one call", fn, n);
    return false;
}
}

extern "C" {
// ---------------------------------------------------------------------------------------------------------------- tiles

int bu_hip_set_pixel_blocks(bu_hip_context* ctx, size_t total_blocks, const bu_pixel_block* blocks) {
    if (!ctx) return 0;
    if (total_blocks > 0xFFFFFFFFull) { set_error(ctx, "too many blocks"); return 0; }
    device_guard g(ctx->device);
    BU_TRY(ctx, ctx->pixel_arena.reserve(total_blocks * sizeof(bu_pixel_block)));
    if (total_blocks) BU_TRY(ctx, h2d(ctx, ctx->pixel_arena.p, blocks, total_blocks * sizeof(bu_pixel_block)));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream)); // the caller may free its copy right after (frontend.cpp:67-79)
    ctx->d_pixel_blocks = ctx->pixel_arena.p;
    ctx->total_blocks = total_blocks;
    return 1;
}

int bu_hip_set_pixel_blocks_device(bu_hip_context* ctx, size_t total_blocks, const void* d_blocks) {
    if (!ctx || total_blocks > 0xFFFFFFFFull) return 0;
    ctx->d_pixel_blocks = d_blocks;
    ctx->total_blocks = total_blocks;
    return 1;
}

const void* bu_hip_get_pixel_blocks_device(const bu_hip_context* ctx, size_t* total_blocks) {
    if (!ctx) return nullptr;
    if (total_blocks) *total_blocks = ctx->total_blocks;
    return ctx->d_pixel_blocks;
}

// ---------------------------------------------------------------------------------------------------------------- section 2

int bu_hip_k_encode_etc1s_blocks(bu_hip_context* ctx, const void* d_px, uint32_t n, int quality, int perceptual, void* d_out) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "encode_etc1s_blocks");
    BU_TRY(ctx, bu::launch_encode_etc1s_blocks(ctx->stream, d_px, n, quality, perceptual != 0, d_out));
    return 1;
}

// Tiles from HOST memory and their first kernel as one pipeline (SURVEY 8d figure (i): the hot path with the host-to-device transfer inside). The upload goes in pieces of
// UP_PIECE_BLOCKS tiles on the context's side stream (the copy engine), the etc1_optimizer kernel of piece i is launched on the main stream behind piece i's event: while piece
// i is encoded, piece i + 1 is on the link and -- for pageable source memory -- pieces i + 2 .. are being copied into the pinned ring by helper threads (one host thread
// copies at 12-17 GB/s, a third of the link). Page-locked source memory is handed to the copy engine as it is. On return h_px may be released (every piece has left it), the
// device side is ordered on the context's stream like any other launch. Same bytes in d_out as bu_hip_k_encode_etc1s_blocks over the uploaded tiles.
int bu_hip_k_upload_and_encode_etc1s_blocks(bu_hip_context* ctx, void* d_px, const void* h_px, uint32_t n, int quality, int perceptual, void* d_out) {
    if (!ctx) return 0;
    if (!n) return 1;
    if (!d_px || !h_px || !d_out) { set_error(ctx, "upload_and_encode_etc1s_blocks: null argument"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n_pieces = (n + UP_PIECE_BLOCKS - 1) / UP_PIECE_BLOCKS;
    // a cooperative host (wait hook) must never block in an event wait, and one piece is no pipeline: upload, then one launch
    if (ctx->wait_hook || n_pieces < 2 || !ensure_side_stream(ctx)) {
        BU_TRY(ctx, h2d(ctx, d_px, h_px, (size_t)n * 64));
        prof_scope ps(ctx, "encode_etc1s_blocks");
        BU_TRY(ctx, bu::launch_encode_etc1s_blocks(ctx->stream, d_px, n, quality, perceptual != 0, d_out));
        return 1;
    }
    while (ctx->up_events.size() < UP_EVENTS) {
        hipEvent_t e = nullptr;
        BU_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->up_events.push_back(e);
    }
    bool pinned_src = false;
    {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, h_px) == hipSuccess) pinned_src = a.type == hipMemoryTypeHost;
        else (void)hipGetLastError();   // ordinary pageable memory is "invalid value" to the runtime: not an error of ours
    }
    const size_t piece_bytes = (size_t)UP_PIECE_BLOCKS * 64;
    if (!pinned_src && ctx->up_ring_cap < piece_bytes * UP_SLOTS) {
        if (ctx->up_ring) { (void)hipHostFree(ctx->up_ring); ctx->up_ring = nullptr; ctx->up_ring_cap = 0; }
        BU_TRY(ctx, hipHostMalloc(&ctx->up_ring, piece_bytes * UP_SLOTS, hipHostMallocDefault));
        ctx->up_ring_cap = piece_bytes * UP_SLOTS;
    }
    // the destination may be a recycled block that earlier launches on the main stream still read: the copies start behind them
    BU_TRY(ctx, hipEventRecord(ctx->side_fork, ctx->stream));
    BU_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
    const char* src = static_cast<const char*>(h_px);
    char* dst = static_cast<char*>(d_px);
    char* out = static_cast<char*>(d_out);
    // pageable source: helper thread t copies pieces t, t + T, ... into ring slot (piece % UP_SLOTS) as soon as the piece that used the slot before has left it
    std::vector<std::atomic<int>> ready(pinned_src ? 0 : n_pieces), issued(pinned_src ? 0 : n_pieces);
    std::atomic<int> stop{0};
    std::vector<std::thread> helpers;
    if (!pinned_src) {
        for (auto& r : ready) r.store(0, std::memory_order_relaxed);
        for (auto& r : issued) r.store(0, std::memory_order_relaxed);
        const unsigned T = std::min<unsigned>(upload_threads(), n_pieces);
        try {
            for (unsigned t = 0; t < T; t++)
                helpers.emplace_back([&, t, T] {
                    (void)hipSetDevice(ctx->device);
                    for (uint32_t i = t; i < n_pieces && !stop.load(std::memory_order_acquire); i += T) {
                        if (i >= UP_SLOTS) {
                            while (!issued[i - UP_SLOTS].load(std::memory_order_acquire)) { if (stop.load(std::memory_order_acquire)) return; std::this_thread::yield(); }
                            (void)hipEventSynchronize(ctx->up_events[(i - UP_SLOTS) % UP_EVENTS]);
                        }
                        const size_t at = (size_t)i * piece_bytes, bytes = std::min(piece_bytes, (size_t)n * 64 - at);
                        std::memcpy(static_cast<char*>(ctx->up_ring) + (size_t)(i % UP_SLOTS) * piece_bytes, src + at, bytes);
                        ready[i].store(1, std::memory_order_release);
                    }
                });
        } catch (...) {
            stop.store(1); for (auto& h : helpers) h.join();
            set_error(ctx, "upload_and_encode_etc1s_blocks: could not start the helper threads");
            return 0;
        }
    }
    hipError_t err = hipSuccess;
    {
        prof_scope ps(ctx, "upload_and_encode_etc1s_blocks");
        for (uint32_t i = 0; i < n_pieces && err == hipSuccess; i++) {
            const size_t at = (size_t)i * piece_bytes, bytes = std::min(piece_bytes, (size_t)n * 64 - at);
            const uint32_t blocks = (uint32_t)(bytes / 64);
            const void* from = src + at;
            if (!pinned_src) {
                while (!ready[i].load(std::memory_order_acquire)) std::this_thread::yield();
                from = static_cast<char*>(ctx->up_ring) + (size_t)(i % UP_SLOTS) * piece_bytes;
            }
            hipEvent_t ev = ctx->up_events[i % UP_EVENTS];
            if ((err = hipMemcpyAsync(dst + at, from, bytes, hipMemcpyHostToDevice, ctx->side_stream)) != hipSuccess) break;
            if ((err = hipEventRecord(ev, ctx->side_stream)) != hipSuccess) break;
            if (!pinned_src) issued[i].store(1, std::memory_order_release);
            if ((err = hipStreamWaitEvent(ctx->stream, ev, 0)) != hipSuccess) break;
            err = bu::launch_encode_etc1s_blocks(ctx->stream, dst + at, blocks, quality, perceptual != 0, out + (size_t)i * UP_PIECE_BLOCKS * 8);
        }
    }
    if (err != hipSuccess) stop.store(1, std::memory_order_release);
    for (auto& h : helpers) h.join();
    // the source (or the ring) must have been read completely before the caller releases it (or the next call refills the ring): the last copy is the one to wait for
    const hipError_t drained = hipStreamSynchronize(ctx->side_stream);
    if (err == hipSuccess) err = drained;
    if (err != hipSuccess) { set_error(ctx, "upload_and_encode_etc1s_blocks: %s", hipGetErrorString(err)); return 0; }
    return 1;
}

int bu_hip_k_endpoint_training_vectors(bu_hip_context* ctx, const void* d_etc, uint32_t n, float* d_out6) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "endpoint_training_vectors");
    BU_TRY(ctx, bu::launch_endpoint_training_vectors(ctx->stream, d_etc, n, d_out6));
    return 1;
}

// The clusters of a codebook fit, split by size: one workgroup per cluster for the many small ones (largest first, so the big ones do not start last), the
// many-workgroup passes of etc1s_codebook_wide.inc for those of bu_hip_tuning::codebook_wide_min texels and more (a sky, a flat wall, a constant alpha plane: one
// workgroup would walk 10^5-10^7 texels 17 times while the rest of the chip waits). `order`: the call's clusters, largest first.
static int codebook_fit_split(bu_hip_context* ctx, const std::vector<uint32_t>& order, const uint32_t* h_offsets, const void* d_px, const void* d_enc, const uint32_t* d_offsets,
                              const uint32_t* d_indices, int quality, bool perceptual, bool forced, uint32_t step, uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid,
                              uint64_t* d_cur_err, const char* label) {
    const uint32_t wide_min = ctx->tuning.codebook_wide_min;
    std::vector<uint32_t> small_ones, big_cluster, big_first, big_sub;
    for (uint32_t c : order) {
        const uint32_t sub = h_offsets[c + 1] - h_offsets[c];
        if (wide_min && sub && (uint64_t)sub * 8u >= wide_min && sub < (1u << 28)) { big_cluster.push_back(c); big_first.push_back(h_offsets[c]); big_sub.push_back(sub); }
        else small_ones.push_back(c);
    }
    std::vector<unsigned char> image;
    bu::cb_wide_layout L{};
    if (!big_cluster.empty()) L = bu::codebook_wide_prepare(big_cluster.data(), big_first.data(), big_sub.data(), (uint32_t)big_cluster.size(), image);
    arena& ord = ctx->scratch[5];
    const size_t ord_bytes = (small_ones.size() * sizeof(uint32_t) + 255) & ~(size_t)255;
    BU_TRY(ctx, ord.reserve(ord_bytes + L.total));
    char* work = static_cast<char*>(ord.p) + ord_bytes;
    if (!small_ones.empty()) BU_TRY(ctx, h2d(ctx, ord.p, small_ones.data(), small_ones.size() * sizeof(uint32_t)));
    if (!image.empty()) BU_TRY(ctx, h2d(ctx, work, image.data(), image.size()));
    {
        prof_scope ps(ctx, label);
        if (!small_ones.empty()) {
            if (forced) BU_TRY(ctx, bu::launch_refit_endpoints_given_selectors(ctx->stream, d_px, d_enc, (uint32_t)small_ones.size(), static_cast<const uint32_t*>(ord.p), d_offsets, d_indices,
                                                                               quality, perceptual, d_params, d_err, d_valid, d_cur_err));
            else BU_TRY(ctx, bu::launch_generate_endpoint_codebook(ctx->stream, d_px, (uint32_t)small_ones.size(), static_cast<const uint32_t*>(ord.p), d_offsets, d_indices,
                                                                   quality, perceptual, step, d_params, d_err, d_valid));
        }
        if (L.n_big) BU_TRY(ctx, bu::launch_codebook_wide(ctx->stream, d_px, d_indices, work, L, quality, perceptual, forced, step, d_enc, d_params, d_err, d_valid, d_cur_err));
    }
    // (no wait here: h2d has copied the uploads' sources into the context's page-locked ring before it returned, and whoever wants the results waits for them)
    return 1;
}

// Test hook: the colour mean the cluster fit starts from (etc.cpp:1034-1041: a running float sum in texel order, divided by the count) of every cluster, through the
// many-workgroup path's order-free evaluation of that sum (etc1s_codebook_wide.inc, cbw_ordered_sum) whatever the clusters' sizes. h_out: 3 floats per cluster.
int bu_hip_k_cluster_colour_means(bu_hip_context* ctx, const void* d_px, uint32_t n_clusters, const uint32_t* h_offsets, const uint32_t* d_indices, float* h_out) {
    if (!ctx) return 0;
    if (!n_clusters) return 1;
    if (!d_px || !h_offsets || !d_indices || !h_out) { set_error(ctx, "cluster_colour_means: null argument"); return 0; }
    device_guard g(ctx->device);
    std::vector<uint32_t> cl(n_clusters), first(n_clusters), sub(n_clusters);
    for (uint32_t c = 0; c < n_clusters; c++) {
        cl[c] = c; first[c] = h_offsets[c]; sub[c] = h_offsets[c + 1] - h_offsets[c];
        if (!sub[c]) { set_error(ctx, "cluster_colour_means: empty cluster %u", c); return 0; }
    }
    std::vector<unsigned char> image;
    const bu::cb_wide_layout L = bu::codebook_wide_prepare(cl.data(), first.data(), sub.data(), n_clusters, image);
    arena& ws = ctx->scratch[5];
    const size_t out_at = (L.total + 255) & ~(size_t)255;
    BU_TRY(ctx, ws.reserve(out_at + (size_t)n_clusters * 12));
    BU_TRY(ctx, h2d(ctx, ws.p, image.data(), image.size()));
    float* d_out = reinterpret_cast<float*>(static_cast<char*>(ws.p) + out_at);
    BU_TRY(ctx, bu::launch_codebook_wide_means(ctx->stream, d_px, d_indices, ws.p, L, d_out));
    if (!fetch(ctx, h_out, d_out, (size_t)n_clusters * 12)) return 0;
    return 1;
}

// The clusters by descending size, ties in index order (= std::stable_sort with that comparator), as an LSD radix sort of the sizes: the device waits while this runs
// (one workgroup per cluster, the big ones must not start last), and the comparison sort of a few thousand indirect keys was 50-80 us of that wait.
static std::vector<uint32_t> size_descending_order(const uint32_t* h_offsets, uint32_t n) {
    std::vector<uint32_t> order(n), tmp(n), key(n);
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) largest = std::max(largest, h_offsets[i + 1] - h_offsets[i]);
    for (uint32_t i = 0; i < n; i++) { order[i] = i; key[i] = largest - (h_offsets[i + 1] - h_offsets[i]); }   // ascending key = descending size
    for (uint32_t shift = 0; shift < 32 && (largest >> shift); shift += 11) {
        uint32_t count[2049] = {};
        for (uint32_t i = 0; i < n; i++) count[((key[order[i]] >> shift) & 2047u) + 1]++;
        for (uint32_t b = 0; b < 2048; b++) count[b + 1] += count[b];
        for (uint32_t i = 0; i < n; i++) tmp[count[(key[order[i]] >> shift) & 2047u]++] = order[i];
        order.swap(tmp);
    }
    return order;
}

int bu_hip_k_generate_endpoint_codebook_part(bu_hip_context* ctx, const void* d_px, uint32_t n_clusters, const uint32_t* h_offsets,
                                             const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual, uint32_t step,
                                             uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint32_t part, uint32_t parts) {
    if (!ctx) return 0;
    if (!n_clusters) return 1;
    if (!parts || part >= parts) { set_error(ctx, "generate_endpoint_codebook: bad part %u of %u", part, parts); return 0; }
    device_guard g(ctx->device);
    // largest clusters first: one workgroup per cluster, so the big ones must not start last. With parts > 1 this call handles the
    // clusters at positions part, part + parts, ... of that order (the same order on every rank: the sort is stable and deterministic).
    const std::vector<uint32_t> order = size_descending_order(h_offsets, n_clusters);
    std::vector<uint32_t> mine;
    for (uint32_t i = part; i < n_clusters; i += parts) mine.push_back(order[i]);
    if (mine.empty()) return 1;
    return codebook_fit_split(ctx, mine, h_offsets, d_px, nullptr, d_offsets, d_indices, quality, perceptual != 0, false, step, d_params, d_err, d_valid, nullptr, "generate_endpoint_codebook");
}

int bu_hip_k_generate_endpoint_codebook(bu_hip_context* ctx, const void* d_px, uint32_t n_clusters, const uint32_t* h_offsets,
                                        const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual, uint32_t step,
                                        uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid) {
    return bu_hip_k_generate_endpoint_codebook_part(ctx, d_px, n_clusters, h_offsets, d_offsets, d_indices, quality, perceptual, step, d_params, d_err, d_valid, 0, 1);
}

int bu_hip_k_refit_endpoints_given_selectors_q(bu_hip_context* ctx, const void* d_px, const void* d_enc, uint32_t n_clusters, const uint32_t* h_offsets,
                                               const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual, uint8_t* d_params, uint64_t* d_err,
                                             uint8_t* d_valid, uint64_t* d_cur_err) {
    if (!ctx) return 0;
    if (!n_clusters) return 1;
    device_guard g(ctx->device);
    const std::vector<uint32_t> order = size_descending_order(h_offsets, n_clusters);
    return codebook_fit_split(ctx, order, h_offsets, d_px, d_enc, d_offsets, d_indices, quality == BU_ETC_QUALITY_SLOW ? BU_ETC_QUALITY_SLOW : BU_ETC_QUALITY_UBER, perceptual != 0, true, 0u,
                              d_params, d_err, d_valid, d_cur_err, "refit_endpoints_given_selectors");
}

int bu_hip_k_refit_endpoints_given_selectors(bu_hip_context* ctx, const void* d_px, const void* d_enc, uint32_t n_clusters, const uint32_t* h_offsets,
                                             const uint32_t* d_offsets, const uint32_t* d_indices, int perceptual, uint8_t* d_params, uint64_t* d_err,
                                             uint8_t* d_valid, uint64_t* d_cur_err) {
    return bu_hip_k_refit_endpoints_given_selectors_q(ctx, d_px, d_enc, n_clusters, h_offsets, d_offsets, d_indices, BU_ETC_QUALITY_UBER, perceptual, d_params, d_err, d_valid, d_cur_err);
}

int bu_hip_k_subblock_errors(bu_hip_context* ctx, const void* d_px, uint32_t n_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                             int perceptual, uint64_t* d_out) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "subblock_errors");
    BU_TRY(ctx, bu::launch_subblock_errors(ctx->stream, d_px, n_blocks, d_block_cluster, d_cluster_params, perceptual != 0, d_out));
    return 1;
}

int bu_hip_k_backend_block_errors(bu_hip_context* ctx, const void* d_px, const void* d_etc_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                                  uint32_t first_block, uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t n_clusters, int perceptual, int with_neighbours,
                                  uint32_t* d_own_err, uint32_t* d_neighbour_err) {
    if (!ctx) return 0;
    if (!d_px || !d_etc_blocks || !d_block_cluster || !d_cluster_params || !d_own_err || (with_neighbours && !d_neighbour_err)) { set_error(ctx, "backend_block_errors: null argument"); return 0; }
    device_guard g(ctx->device);
    prof_scope ps(ctx, "backend_block_errors");
    BU_TRY(ctx, bu::launch_backend_block_errors(ctx->stream, d_px, d_etc_blocks, d_block_cluster, d_cluster_params, first_block, num_blocks_x, num_blocks_y, n_clusters, perceptual != 0,
                                                with_neighbours != 0, d_own_err, d_neighbour_err));
    return 1;
}

int bu_hip_k_refine_endpoint_clusterization(bu_hip_context* ctx, const void* d_px, uint32_t n_blocks, const uint32_t* d_block_cluster,
                                            const uint8_t* d_cluster_params, uint32_t n_clusters, uint32_t n_parents, const uint32_t* d_cand_offsets,
                                            const uint32_t* d_cand_indices, const uint8_t* d_block_parent, int perceptual, uint32_t* d_out_best) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    void* work = nullptr;
    const int path = bu_hip_refine_path(ctx, n_clusters, n_parents, perceptual);
    if (path != 1) { BU_TRY(ctx, ctx->refine_lists.reserve(bu::refine_workspace_bytes(n_clusters, n_parents, n_blocks))); work = ctx->refine_lists.p; }
    prof_scope ps(ctx, "refine_endpoint_clusterization");
    BU_TRY(ctx, bu::launch_refine_endpoint_clusterization(ctx->stream, d_px, n_blocks, d_block_cluster, d_cluster_params, n_clusters, n_parents,
                                                          d_cand_offsets, d_cand_indices, d_block_parent, perceptual != 0, d_out_best, path, work));
    return 1;
}

int bu_hip_refine_path(const bu_hip_context* ctx, uint32_t n_clusters, uint32_t n_parents, int perceptual) {
    bu_hip_tuning t;
    bu_hip_get_tuning(ctx, &t, sizeof(t));   // a null context: the process defaults
    return bu::refine_path(t.refine_unsorted, n_clusters, n_parents, perceptual != 0);
}

int bu_hip_k_extract_blocks(bu_hip_context* ctx, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out) {
    if (!ctx) return 0;
    if (!d_rgba || !d_out || !width || !height || pitch_bytes < width * 4u) { set_error(ctx, "extract_blocks: bad arguments"); return 0; }
    device_guard g(ctx->device);
    prof_scope ps(ctx, "extract_blocks");
    BU_TRY(ctx, bu::launch_extract_blocks(ctx->stream, d_rgba, width, height, pitch_bytes, d_out));
    return 1;
}

int bu_hip_k_extract_slices(bu_hip_context* ctx, const bu_hip_slice_source* slices, uint32_t n, void* d_out) {
    if (!ctx) return 0;
    static const char* const fn = "extract_slices";
    // the records as they are, then the table of where each slice's tiles begin among the tiles of the call
    bu::slice_table table;
    if (!checked(ctx, [&](bu::err_text e) { return bu::build_source_slices(table, fn, slices, n, d_out, e); })) return 0;
    device_guard g(ctx->device);
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    prof_scope ps(ctx, fn);
    BU_TRY(ctx, bu::launch_extract_slices(ctx->stream, static_cast<const bu_hip_slice_source*>(d.records), d.prefix, n, table.total, d_out));
    return 1;
}

int bu_hip_k_resample_rgba8(bu_hip_context* ctx, const void* d_src, uint32_t src_w, uint32_t src_h, void* d_dst, uint32_t dst_w, uint32_t dst_h,
                            const uint32_t* x_first, const uint16_t* x_pixel, const float* x_weight, const uint32_t* y_first, const uint16_t* y_pixel, const float* y_weight,
                            int x_after_y, int srgb, const float* srgb_to_linear, const uint8_t* linear_to_srgb, uint32_t num_comps) {
    if (!ctx) return 0;
    if (!d_src || !d_dst || !src_w || !src_h || !dst_w || !dst_h || !x_first || !x_pixel || !x_weight || !y_first || !y_pixel || !y_weight || !srgb_to_linear ||
        !linear_to_srgb || num_comps < 3 || num_comps > 4 || src_w > 16384 || src_h > 16384) { set_error(ctx, "resample_rgba8: bad arguments"); return 0; }
    device_guard g(ctx->device);
    // everything the kernels read besides the image, packed into one upload: lists of both axes, then the tables
    const size_t nx = x_first[dst_w], ny = y_first[dst_h];
    for (uint32_t i = 0; i < nx; i++) if (x_pixel[i] >= src_w) { set_error(ctx, "resample_rgba8: x contributor out of range"); return 0; }
    for (uint32_t i = 0; i < ny; i++) if (y_pixel[i] >= src_h) { set_error(ctx, "resample_rgba8: y contributor out of range"); return 0; }
    auto pad = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_xf = 0, o_xw = pad(o_xf + (dst_w + 1) * 4), o_xp = pad(o_xw + nx * 4), o_yf = pad(o_xp + nx * 2), o_yw = pad(o_yf + (dst_h + 1) * 4), o_yp = pad(o_yw + ny * 4),
                 o_t0 = pad(o_yp + ny * 2), o_t1 = o_t0 + 1024, total = o_t1 + 8192;
    std::vector<uint8_t> pack(total, 0);
    std::memcpy(&pack[o_xf], x_first, (dst_w + 1) * 4); std::memcpy(&pack[o_xw], x_weight, nx * 4); std::memcpy(&pack[o_xp], x_pixel, nx * 2);
    std::memcpy(&pack[o_yf], y_first, (dst_h + 1) * 4); std::memcpy(&pack[o_yw], y_weight, ny * 4); std::memcpy(&pack[o_yp], y_pixel, ny * 2);
    std::memcpy(&pack[o_t0], srgb_to_linear, 1024); std::memcpy(&pack[o_t1], linear_to_srgb, 8192);
    arena &lists = ctx->scratch[4], &tmp = ctx->scratch[5];
    const size_t tmp_px = std::max((size_t)dst_w * src_h, (size_t)src_w * dst_h);
    BU_TRY(ctx, lists.reserve(total));
    BU_TRY(ctx, tmp.reserve(tmp_px * 16));
    BU_TRY(ctx, h2d(ctx, lists.p, pack.data(), total));
    const char* b = static_cast<const char*>(lists.p);
    {
        prof_scope ps(ctx, "resample_rgba8");
        BU_TRY(ctx, bu::launch_resample_rgba8(ctx->stream, d_src, src_w, src_h, d_dst, dst_w, dst_h, (const uint32_t*)(b + o_xf), (const uint16_t*)(b + o_xp), (const float*)(b + o_xw),
                                              (const uint32_t*)(b + o_yf), (const uint16_t*)(b + o_yp), (const float*)(b + o_yw), x_after_y != 0, srgb != 0,
                                              (const float*)(b + o_t0), (const uint8_t*)(b + o_t1), num_comps, tmp.p));
    }
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));  // the packed lists are reused by the next call
    return 1;
}

int bu_hip_k_determine_selectors(bu_hip_context* ctx, const void* d_px, uint32_t n_blocks, const uint8_t* d_color5_inten,
                                 const uint32_t* d_block_cluster, int perceptual, void* d_out) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "determine_selectors");
    BU_TRY(ctx, bu::launch_determine_selectors(ctx->stream, d_px, n_blocks, d_color5_inten, d_block_cluster, perceptual != 0, d_out));
    return 1;
}

int bu_hip_k_selector_training_vectors(bu_hip_context* ctx, const void* d_enc, uint32_t n_blocks, int perceptual, float* d_out16, uint64_t* d_w) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "selector_training_vectors");
    BU_TRY(ctx, bu::launch_selector_training_vectors(ctx->stream, d_enc, n_blocks, perceptual != 0, d_out16, d_w));
    return 1;
}

int bu_hip_k_create_optimized_selector_codebook(bu_hip_context* ctx, const void* d_px, const void* d_enc, uint32_t n_clusters,
                                                const uint32_t* d_offsets, const uint32_t* d_block_indices, int perceptual, void* d_selector_blocks) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    if (!n_clusters) return 1;
    // (no look at the offsets from here: the accumulation kernel is a fixed number of waves that find the span on the device)
    arena& ws = ctx->scratch[4];
    BU_TRY(ctx, ws.reserve(bu::create_optimized_selector_codebook_workspace_bytes(n_clusters)));
    prof_scope ps(ctx, "create_optimized_selector_codebook");
    BU_TRY(ctx, bu::launch_create_optimized_selector_codebook(ctx->stream, d_px, d_enc, n_clusters, d_offsets, d_block_indices, perceptual != 0, ws.p,
                                                              d_selector_blocks));
    return 1;
}

int bu_hip_k_find_optimal_selector_clusters(bu_hip_context* ctx, const void* d_px, void* d_enc, uint32_t n_blocks, const void* d_selector_blocks,
                                            uint32_t n_selectors, uint32_t n_parents, const uint32_t* d_cand_offsets, const uint32_t* d_cand_indices,
                                            const uint8_t* d_block_parent, int perceptual, uint32_t chunk, uint32_t* d_out) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "find_optimal_selector_clusters");
    arena& tmp = ctx->scratch[4];
    // behind the per-block scratch: room for the candidates' selector words in list order (at most parents x selectors of them; left out beyond 64 MiB)
    const size_t idx_bytes = ((size_t)n_blocks * sizeof(uint32_t) + 255) & ~(size_t)255;
    size_t words = (size_t)(n_parents ? n_parents : 1u) * n_selectors;
    if (words * 4 > ((size_t)64 << 20)) words = 0;
    BU_TRY(ctx, tmp.reserve(idx_bytes + words * 4));
    BU_TRY(ctx, bu::launch_find_optimal_selector_clusters(ctx->stream, d_px, d_enc, n_blocks, d_selector_blocks, n_selectors, n_parents, d_cand_offsets,
                                                          d_cand_indices, d_block_parent, perceptual != 0, chunk, static_cast<uint32_t*>(tmp.p), d_out,
                                                          words ? reinterpret_cast<uint32_t*>(static_cast<char*>(tmp.p) + idx_bytes) : nullptr, words));
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------- cluster bookkeeping on the device

int bu_hip_k_map_blocks_from_groups(bu_hip_context* ctx, const uint32_t* d_goffs, const uint32_t* d_idx, uint32_t n, uint32_t u_total, const uint32_t* d_leaf,
                                    const uint32_t* d_first_pos, const uint32_t* d_parent_of_unique, uint32_t* d_cluster, uint32_t* d_pos, uint8_t* d_parent) {
    if (!ctx) return 0;
    if (n && (!d_goffs || !d_idx || !d_leaf || !d_cluster || (d_pos && !d_first_pos))) { set_error(ctx, "map_blocks_from_groups: null pointer"); return 0; }
    device_guard g(ctx->device);
    prof_scope ps(ctx, "map_blocks_from_groups");
    BU_TRY(ctx, bu::launch_blocks_from_groups(ctx->stream, d_goffs, d_idx, n, u_total, d_leaf, d_first_pos, d_parent_of_unique, d_cluster, d_pos, d_parent));
    return 1;
}

int bu_hip_k_map_rank_blocks(bu_hip_context* ctx, const uint32_t* d_cluster, uint32_t n, uint32_t k, uint32_t* d_sizes, uint32_t* d_offsets, uint32_t* d_sorted, uint32_t* d_pos) {
    if (!ctx) return 0;
    if (n && (!d_cluster || !d_sizes || !d_offsets || !d_sorted)) { set_error(ctx, "map_rank_blocks: null pointer"); return 0; }
    if (!sort_size_ok(ctx, "map_rank_blocks", n)) return 0;
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[4];
    BU_TRY(ctx, ws.reserve(bu::rank_blocks_workspace_bytes(n, k)));
    prof_scope ps(ctx, "map_rank_blocks");
    BU_TRY(ctx, bu::launch_rank_blocks(ctx->stream, d_cluster, n, k, ws.p, d_sizes, d_offsets, d_sorted, d_pos));
    return 1;
}

int bu_hip_k_map_endpoint_csr(bu_hip_context* ctx, const uint32_t* d_cluster, const uint32_t* d_pos, uint32_t n, const uint32_t* d_offsets, uint32_t* d_indices) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "map_endpoint_csr");
    BU_TRY(ctx, bu::launch_endpoint_csr_fill(ctx->stream, d_cluster, d_pos, n, d_offsets, d_indices));
    return 1;
}

int bu_hip_k_map_remap(bu_hip_context* ctx, uint32_t* d_cluster, uint32_t* d_pos, uint32_t n, const uint32_t* d_new_index, const uint32_t* d_base) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_scope ps(ctx, "map_remap");
    BU_TRY(ctx, bu::launch_remap_clusters(ctx->stream, d_cluster, d_pos, n, d_new_index, d_base));
    return 1;
}

int bu_hip_k_map_count_differences(bu_hip_context* ctx, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, uint32_t* d_count) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    BU_TRY(ctx, bu::launch_count_differences(ctx->stream, d_a, d_b, n, d_count));
    return 1;
}

int bu_hip_k_map_membership(bu_hip_context* ctx, const uint8_t* d_parent, const uint32_t* d_cluster, uint32_t n, uint32_t parents, uint32_t clusters, uint8_t* d_flags) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    BU_TRY(ctx, bu::launch_membership(ctx->stream, d_parent, d_cluster, n, parents, clusters, d_flags));
    return 1;
}

int bu_hip_k_map_gather(bu_hip_context* ctx, const uint32_t* d_table, const uint32_t* d_index, uint32_t n, uint32_t* d_out) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    BU_TRY(ctx, bu::launch_gather_u32(ctx->stream, d_table, d_index, n, d_out));
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------- f3: k-means codebooks (fast mode)

int bu_hip_kmeans_codebook(bu_hip_context* ctx, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_goffs, uint32_t n, uint32_t max_clusters,
                           uint32_t n_parents, uint32_t iterations, uint32_t* d_cluster, uint32_t* d_parent, uint32_t* out_clusters, uint32_t* out_parents) {
    if (!ctx) return 0;
    if (!d_keys || !d_cluster || !out_clusters || !n || !max_clusters || (kind == 0 && !d_weights) || (kind != 0 && !d_goffs) || (n_parents && !d_parent)) {
        set_error(ctx, "kmeans_codebook: bad arguments");
        return 0;
    }
    device_guard g(ctx->device);
    const uint32_t k = std::min(max_clusters, n);
    arena& ws = ctx->scratch[3];
    BU_TRY(ctx, ws.reserve(bu::kmeans_workspace_bytes(n, k) + (size_t)k * 8 + 256));
    const bu::kmeans_buffers b = bu::kmeans_carve(ws.p, n, k);
    uint32_t* d_tab = reinterpret_cast<uint32_t*>(static_cast<char*>(ws.p) + bu::kmeans_workspace_bytes(n, k));
    {
        prof_scope ps(ctx, kind ? "kmeans_endpoints" : "kmeans_selectors");
        BU_TRY(ctx, bu::launch_kmeans(ctx->stream, kind, d_keys, d_weights, d_goffs, n, k, iterations, b, d_cluster));
    }
    std::vector<uint64_t> sums((size_t)k * 17);
    std::vector<float> cen((size_t)k * 16);
    {
        mail_fetch f(ctx);
        BU_TRY(ctx, f.add(sums.data(), b.sums, sums.size() * 8));
        BU_TRY(ctx, f.add(cen.data(), b.cen, cen.size() * 4));
        if (!f.wait()) return 0;
    }
    // non-empty clusters, in index order
    std::vector<uint32_t> old_to_new(k, 0), live;
    for (uint32_t c = 0; c < k; c++) if (sums[(size_t)c * 17 + 16]) { old_to_new[c] = (uint32_t)live.size(); live.push_back(c); }
    const uint32_t kl = (uint32_t)live.size();
    *out_clusters = kl;
    uint32_t parents = 0;
    std::vector<uint32_t> parent_of_old(k, 0);
    if (n_parents && kl) {
        // the parent level: weighted k-means over the live clusters' final centres (the true means of their members), a few thousand points, on the host
        const int D = 16;
        std::vector<double> pts((size_t)kl * D), wts(kl);
        for (uint32_t i = 0; i < kl; i++) {
            const uint64_t w = sums[(size_t)live[i] * 17 + 16];
            wts[i] = (double)w;
            for (int d = 0; d < D; d++) pts[(size_t)i * D + d] = (double)sums[(size_t)live[i] * 17 + d] / (double)w;
        }
        const uint32_t P = std::min(n_parents, kl);
        std::vector<double> pc((size_t)P * D);
        for (uint32_t p = 0; p < P; p++) std::memcpy(&pc[(size_t)p * D], &pts[(size_t)(((uint64_t)p * 2 + 1) * kl / (2ull * P)) * D], D * sizeof(double));
        std::vector<uint32_t> owner(kl, 0);
        for (int it = 0; it < 12; it++) {
            for (uint32_t i = 0; i < kl; i++) {
                double bd = 1e300; uint32_t bp = 0;
                for (uint32_t p = 0; p < P; p++) {
                    double dd = 0;
                    for (int d = 0; d < D; d++) { const double t = pts[(size_t)i * D + d] - pc[(size_t)p * D + d]; dd += t * t; }
                    if (dd < bd) { bd = dd; bp = p; }
                }
                owner[i] = bp;
            }
            std::vector<double> acc((size_t)P * D, 0.0), aw(P, 0.0);
            for (uint32_t i = 0; i < kl; i++) { aw[owner[i]] += wts[i]; for (int d = 0; d < D; d++) acc[(size_t)owner[i] * D + d] += wts[i] * pts[(size_t)i * D + d]; }
            for (uint32_t p = 0; p < P; p++) if (aw[p] > 0) for (int d = 0; d < D; d++) pc[(size_t)p * D + d] = acc[(size_t)p * D + d] / aw[p];
        }
        std::vector<int32_t> renum(P, -1);   // parents that own something, in index order
        for (uint32_t i = 0; i < kl; i++) if (renum[owner[i]] < 0) renum[owner[i]] = 0;
        for (uint32_t p = 0; p < P; p++) if (renum[p] == 0) renum[p] = (int32_t)parents++;
        for (uint32_t i = 0; i < kl; i++) parent_of_old[live[i]] = (uint32_t)renum[owner[i]];
    }
    if (out_parents) *out_parents = parents;
    // per distinct vector: parent first (from the raw assignment), then the compacted cluster index in place
    if (n_parents) {
        BU_TRY(ctx, h2d(ctx, d_tab, parent_of_old.data(), (size_t)k * 4));
        BU_TRY(ctx, bu::launch_gather_u32(ctx->stream, d_tab, d_cluster, n, d_parent));
    }
    BU_TRY(ctx, h2d(ctx, d_tab + k, old_to_new.data(), (size_t)k * 4));
    BU_TRY(ctx, bu::launch_gather_u32(ctx->stream, d_tab + k, d_cluster, n, d_cluster));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    (void)cen;
    return 1;
}

// the steps of the call above one at a time (kernel-level tests): the same functions launch_kmeans is made of, on the same workspace
int bu_hip_k_kmeans_seed(bu_hip_context* ctx, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_goffs, uint32_t n, uint32_t k, uint32_t* d_pick,
                         float* d_centroids) {
    if (!ctx) return 0;
    if (!d_keys || !d_pick || !d_centroids || !n || !k || k > n || (kind == 0 && !d_weights) || (kind != 0 && !d_goffs)) {
        set_error(ctx, "kmeans_seed: bad arguments");
        return 0;
    }
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[3];
    BU_TRY(ctx, ws.reserve(bu::kmeans_workspace_bytes(n, k)));
    const bu::kmeans_buffers b = bu::kmeans_carve(ws.p, n, k);
    const uint64_t* weights = nullptr;
    BU_TRY(ctx, bu::kmeans_begin(ctx->stream, kind, d_keys, d_weights, d_goffs, n, b, &weights));
    bu::kmeans_seed(ctx->stream, n, k, b);
    BU_TRY(ctx, hipGetLastError());
    BU_TRY(ctx, hipMemcpyAsync(d_pick, b.pick, (size_t)k * 4, hipMemcpyDeviceToDevice, ctx->stream));
    BU_TRY(ctx, hipMemcpyAsync(d_centroids, b.cen, (size_t)k * 16 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return 1;
}

int bu_hip_k_kmeans_round(bu_hip_context* ctx, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_goffs, uint32_t n, uint32_t k, float* d_centroids,
                          uint64_t* d_live, int update, uint32_t* d_assign, uint64_t* d_sums, uint64_t* d_worst) {
    if (!ctx) return 0;
    if (!d_keys || !d_centroids || !d_assign || !d_sums || !n || !k || k > n || (kind == 0 && !d_weights) || (kind != 0 && !d_goffs) || (update && !d_live)) {
        set_error(ctx, "kmeans_round: bad arguments");
        return 0;
    }
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[3];
    BU_TRY(ctx, ws.reserve(bu::kmeans_workspace_bytes(n, k)));
    const bu::kmeans_buffers b = bu::kmeans_carve(ws.p, n, k);
    hipStream_t st = ctx->stream;
    const uint64_t* weights = nullptr;
    BU_TRY(ctx, bu::kmeans_begin(st, kind, d_keys, d_weights, d_goffs, n, b, &weights));
    bu::kmeans_flags(st, kind, n, k, b);
    BU_TRY(ctx, hipMemcpyAsync(b.cen, d_centroids, (size_t)k * 16 * 4, hipMemcpyDeviceToDevice, st));
    // the live word of cluster c is where the rounds keep it: the weight word of its sums
    if (d_live) bu::kmeans_set_live(st, d_live, k, b);
    BU_TRY(ctx, bu::kmeans_assign_round(st, kind, weights, n, k, b, d_live != nullptr, update || d_worst, d_assign, 0));
    BU_TRY(ctx, hipMemcpyAsync(d_sums, b.sums, (size_t)k * 17 * 8, hipMemcpyDeviceToDevice, st));
    if (d_worst) BU_TRY(ctx, hipMemcpyAsync(d_worst, bu::kmeans_wg_worst(b), (size_t)bu::kmeans_workgroups(n) * 8, hipMemcpyDeviceToDevice, st));
    if (update) {
        BU_TRY(ctx, bu::kmeans_update_round(st, n, k, b));
        BU_TRY(ctx, hipMemcpyAsync(d_centroids, b.cen, (size_t)k * 16 * 4, hipMemcpyDeviceToDevice, st));
        bu::kmeans_get_live(st, d_live, k, b);
    }
    BU_TRY(ctx, hipGetLastError());
    return 1;
}

int bu_hip_k_unique_endpoint_vectors(bu_hip_context* ctx, const void* d_etc1_blocks, uint32_t n_blocks, uint32_t* d_sorted_block_idx, uint64_t* d_unique_keys,
                                     uint32_t* d_group_offsets, uint32_t* out_unique) {
    if (!ctx) return 0;
    if (!out_unique || (n_blocks && (!d_etc1_blocks || !d_sorted_block_idx || !d_unique_keys || !d_group_offsets))) { set_error(ctx, "unique_endpoint_vectors: null pointer"); return 0; }
    *out_unique = 0;
    if (!n_blocks) return 1;
    if (!sort_size_ok(ctx, "unique_endpoint_vectors", n_blocks)) return 0;
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[4];
    BU_TRY(ctx, ws.reserve(bu::unique_endpoint_vectors_workspace_bytes(n_blocks)));
    uint32_t* d_n = nullptr;
    {
        prof_scope ps(ctx, "unique_endpoint_vectors");
        BU_TRY(ctx, bu::launch_unique_endpoint_vectors(ctx->stream, d_etc1_blocks, n_blocks, ws.p, d_sorted_block_idx, d_unique_keys, d_group_offsets, &d_n));
    }
    if (!fetch(ctx, out_unique, d_n, 4)) return 0;
    return 1;
}

int bu_hip_k_unique_selector_vectors(bu_hip_context* ctx, const void* d_enc_blocks, const uint64_t* d_weights, uint32_t n_blocks, uint32_t* d_sorted_block_idx,
                                     uint32_t* d_unique_keys, uint64_t* d_unique_weights, uint32_t* d_group_offsets, uint32_t* out_unique) {
    if (!ctx) return 0;
    if (!out_unique || (n_blocks && (!d_enc_blocks || !d_weights || !d_sorted_block_idx || !d_unique_keys || !d_unique_weights || !d_group_offsets))) {
        set_error(ctx, "unique_selector_vectors: null pointer");
        return 0;
    }
    *out_unique = 0;
    if (!n_blocks) return 1;
    if (!sort_size_ok(ctx, "unique_selector_vectors", n_blocks)) return 0;
    device_guard g(ctx->device);
    arena& ws = ctx->scratch[4];
    BU_TRY(ctx, ws.reserve(bu::unique_selector_vectors_workspace_bytes(n_blocks)));
    uint32_t* d_n = nullptr;
    {
        prof_scope ps(ctx, "unique_selector_vectors");
        BU_TRY(ctx, bu::launch_unique_selector_vectors(ctx->stream, d_enc_blocks, d_weights, n_blocks, ws.p, d_sorted_block_idx, d_unique_keys, d_unique_weights,
                                                        d_group_offsets, &d_n));
    }
    if (!fetch(ctx, out_unique, d_n, 4)) return 0;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------- section 1 (blocking, host pointers)

int bu_hip_encode_etc1s_blocks(bu_hip_context* ctx, bu_etc_block* out, int perceptual, uint32_t total_perms) {
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    arena& o = ctx->scratch[0];
    BU_TRY(ctx, o.reserve((size_t)n * 8));
    BU_TRY(ctx, bu::launch_encode_etc1s_blocks(ctx->stream, ctx->d_pixel_blocks, n, quality_from_perms(total_perms), perceptual != 0, o.p));
    if (!fetch(ctx, out, o.p, (size_t)n * 8)) return 0;
    return 1;
}

int bu_hip_determine_selectors(bu_hip_context* ctx, const bu_color_rgba* color5_inten, bu_etc_block* out, int perceptual) {
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    arena &in = ctx->scratch[0], &o = ctx->scratch[1];
    BU_TRY(ctx, in.reserve((size_t)n * 4));
    BU_TRY(ctx, o.reserve((size_t)n * 8));
    BU_TRY(ctx, h2d(ctx, in.p, color5_inten, (size_t)n * 4));
    BU_TRY(ctx, bu::launch_determine_selectors(ctx->stream, ctx->d_pixel_blocks, n, static_cast<const uint8_t*>(in.p), nullptr, perceptual != 0, o.p));
    if (!fetch(ctx, out, o.p, (size_t)n * 8)) return 0;
    return 1;
}

int bu_hip_refine_endpoint_clusterization(bu_hip_context* ctx, const bu_block_info* info, uint32_t total_clusters, const bu_endpoint_cluster* clusters,
                                          const uint32_t* /*sorted_block_indices*/, uint32_t* out, int perceptual) {
    // The reference seam passes, per block, a window [first_cluster_ofs, first_cluster_ofs+num_clusters) into a flat list of
    // {unscaled colour, inten, cluster index} (frontend.cpp:1684-1750). host/seam_translate.h turns that into the device layer's form:
    // a parameter table addressed by POSITION in the flat list, one "parent" per distinct window. The block's current
    // cluster is identified by its index value; the kernel's tie rule compares against the candidate's position, so the
    // position of the current cluster inside the window is looked up there.
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    if (n && !out) { set_error(ctx, "refine: null pointer"); return 0; }
    bu::seam::refine_tables t;
    if (const char* e = bu::seam::translate_refine(info, n, total_clusters, clusters, t)) { set_error(ctx, "%s", e); return 0; }
    if (!n) return 1;
    const uint32_t n_parents = t.win.n_parents();

    arena &a_par = ctx->scratch[0], &a_cur = ctx->scratch[1], &a_off = ctx->scratch[2], &a_idx = ctx->scratch[3], &a_out = ctx->scratch[4];
    arena& a_bp = ctx->scratch[5];
    BU_TRY(ctx, a_par.reserve(total_clusters * 4ull)); BU_TRY(ctx, a_cur.reserve(n * 4ull)); BU_TRY(ctx, a_off.reserve(t.win.cand_offsets.size() * 4ull));
    BU_TRY(ctx, a_idx.reserve(t.win.cand_indices.size() * 4ull + 4)); BU_TRY(ctx, a_out.reserve(n * 4ull)); BU_TRY(ctx, a_bp.reserve(n));
    BU_TRY(ctx, h2d(ctx, a_par.p, t.params.data(), total_clusters * 4ull));
    BU_TRY(ctx, h2d(ctx, a_cur.p, t.block_cur.data(), n * 4ull));
    BU_TRY(ctx, h2d(ctx, a_off.p, t.win.cand_offsets.data(), t.win.cand_offsets.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_idx.p, t.win.cand_indices.data(), t.win.cand_indices.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_bp.p, t.win.block_parent.data(), n));
    void* work = nullptr;
    const int path = bu_hip_refine_path(ctx, total_clusters, n_parents, perceptual);
    if (path != 1) { BU_TRY(ctx, ctx->refine_lists.reserve(bu::refine_workspace_bytes(total_clusters, n_parents, n))); work = ctx->refine_lists.p; }
    BU_TRY(ctx, bu::launch_refine_endpoint_clusterization(ctx->stream, ctx->d_pixel_blocks, n, static_cast<const uint32_t*>(a_cur.p),
                                                          static_cast<const uint8_t*>(a_par.p), total_clusters, n_parents,
                                                          static_cast<const uint32_t*>(a_off.p), static_cast<const uint32_t*>(a_idx.p),
                                                          static_cast<const uint8_t*>(a_bp.p), perceptual != 0, static_cast<uint32_t*>(a_out.p), path, work));
    std::vector<uint32_t> pos(n);
    if (!fetch(ctx, pos.data(), a_out.p, n * 4ull)) return 0;
    for (uint32_t b = 0; b < n; b++) out[b] = clusters[pos[b]].m_cluster_index; // positions -> cluster indices (.cl:1150)
    return 1;
}

int bu_hip_find_optimal_selector_clusters_for_each_block(bu_hip_context* ctx, const bu_fosc_block* info, uint32_t total_input_selectors,
                                                         const bu_fosc_selector* selectors, const uint32_t* selector_cluster_indices, uint32_t* out, int perceptual) {
    if (!ctx || !ctx->d_pixel_blocks) { if (ctx) set_error(ctx, "no pixel blocks set"); return 0; }
    device_guard g(ctx->device);
    const uint32_t n = (uint32_t)ctx->total_blocks;
    if (n && (!out || !selector_cluster_indices)) { set_error(ctx, "fosc: null pointer"); return 0; }
    // packed 2-bit selectors -> etc_block selector bytes addressed by position in the flat list, colour5 + inten -> etc_block, windows -> parents
    bu::seam::fosc_tables t;
    if (const char* e = bu::seam::translate_fosc(info, n, total_input_selectors, selectors, t)) { set_error(ctx, "%s", e); return 0; }
    if (!n) return 1;
    const uint32_t n_parents = t.win.n_parents();

    arena &a_sel = ctx->scratch[0], &a_enc = ctx->scratch[1], &a_off = ctx->scratch[2], &a_idx = ctx->scratch[3], &a_tmp = ctx->scratch[4], &a_bp = ctx->scratch[5];
    BU_TRY(ctx, a_sel.reserve(total_input_selectors * 8ull + 8)); BU_TRY(ctx, a_enc.reserve(n * 8ull + n * 4ull)); BU_TRY(ctx, a_off.reserve(t.win.cand_offsets.size() * 4ull));
    BU_TRY(ctx, a_idx.reserve(t.win.cand_indices.size() * 4ull + 4)); BU_TRY(ctx, a_tmp.reserve(n * 4ull)); BU_TRY(ctx, a_bp.reserve(n));
    uint32_t* d_out = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(a_enc.p) + n * 8ull);
    BU_TRY(ctx, h2d(ctx, a_sel.p, t.selector_blocks.data(), total_input_selectors * 8ull));
    BU_TRY(ctx, h2d(ctx, a_enc.p, t.encoded_blocks.data(), n * 8ull));
    BU_TRY(ctx, h2d(ctx, a_off.p, t.win.cand_offsets.data(), t.win.cand_offsets.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_idx.p, t.win.cand_indices.data(), t.win.cand_indices.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_bp.p, t.win.block_parent.data(), n));
    // chunk = 0: the OpenCL seam has no "same tile as previous block" shortcut (ocl_kernels.cl:1159-1225)
    BU_TRY(ctx, bu::launch_find_optimal_selector_clusters(ctx->stream, ctx->d_pixel_blocks, a_enc.p, n, a_sel.p, total_input_selectors, n_parents,
                                                          static_cast<const uint32_t*>(a_off.p), static_cast<const uint32_t*>(a_idx.p), static_cast<const uint8_t*>(a_bp.p),
                                                          perceptual != 0, 0, static_cast<uint32_t*>(a_tmp.p), d_out, nullptr, 0));
    std::vector<uint32_t> pos(n);
    if (!fetch(ctx, pos.data(), d_out, n * 4ull)) return 0;
    for (uint32_t b = 0; b < n; b++) out[b] = selector_cluster_indices[pos[b]];
    return 1;
}

int bu_hip_encode_etc1s_pixel_clusters(bu_hip_context* ctx, bu_etc_block* out, uint32_t total_clusters, const bu_pixel_cluster* clusters,
                                       uint64_t total_pixels, const bu_color_rgba* pixels, const uint32_t* weights, int perceptual, uint32_t total_perms) {
    // The reference seam hands over de-duplicated colours with multiplicities. The device layer works on unweighted pixel lists
    // (bu_hip_k_generate_endpoint_codebook, which is what our own frontend uses and what INTEGRATION.md binds). For the legacy
    // call the multiplicities are expanded into a temporary tile array laid out as "training vectors" of 8 pixels; clusters whose
    // expanded size is not a multiple of 8 are REPEATED whole (host/seam_translate.h, translate_pixel_clusters, has the argument).
    if (!ctx) return 0;
    device_guard g(ctx->device);
    if (!total_clusters) return 1;
    if (!out) { set_error(ctx, "pixel clusters: null pointer"); return 0; }
    bu::seam::pixel_tables t;
    if (const char* e = bu::seam::translate_pixel_clusters(total_clusters, clusters, total_pixels, pixels, weights, t)) { set_error(ctx, "%s", e); return 0; }
    arena &a_px = ctx->scratch[0], &a_off = ctx->scratch[1], &a_idx = ctx->scratch[2], &a_par = ctx->scratch[3];
    const size_t params_bytes = ((total_clusters * 4ull + 7) / 8) * 8;
    BU_TRY(ctx, a_px.reserve(t.texels.size() * 4ull)); BU_TRY(ctx, a_off.reserve(t.offsets.size() * 4ull)); BU_TRY(ctx, a_idx.reserve(t.indices.size() * 4ull + 4));
    BU_TRY(ctx, a_par.reserve(params_bytes + total_clusters * 8ull + total_clusters));
    BU_TRY(ctx, h2d(ctx, a_px.p, t.texels.data(), t.texels.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_off.p, t.offsets.data(), t.offsets.size() * 4ull));
    BU_TRY(ctx, h2d(ctx, a_idx.p, t.indices.data(), t.indices.size() * 4ull));
    uint8_t* d_params = static_cast<uint8_t*>(a_par.p);
    uint64_t* d_err = reinterpret_cast<uint64_t*>(d_params + params_bytes);
    uint8_t* d_valid = reinterpret_cast<uint8_t*>(d_err + total_clusters);
    // the cluster fit has no FAST quality (frontend.cpp:1530-1533): total_perms = 4 is fitted as 16
    if (!bu_hip_k_generate_endpoint_codebook(ctx, a_px.p, total_clusters, t.offsets.data(), static_cast<const uint32_t*>(a_off.p), static_cast<const uint32_t*>(a_idx.p),
                                             std::max(quality_from_perms(total_perms), (int)bu::BU_Q_MEDIUM), perceptual, 0, d_params, d_err, d_valid))
        return 0;
    std::vector<uint8_t> params(total_clusters * 4ull);
    if (!fetch(ctx, params.data(), d_params, params.size())) return 0;
    for (uint32_t c = 0; c < total_clusters; c++) {
        const uint64_t m = bu::seam::color5_inten_to_etc_block(params[c * 4], params[c * 4 + 1], params[c * 4 + 2], params[c * 4 + 3]);
        memcpy(&out[c], &m, 8);
    }
    return 1;
}
} // extern "C"
