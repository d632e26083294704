// api_internal.h -- context management and the C ABI of libbasisu_hip.so (include/basisu_hip.h): what its units (api_context / api_etc1s / api_tsvq / api_uastc .cpp) share.
// Replaces encoder/basisu_opencl.cpp of the reference: same entry points, same ownership and error conventions
// (opencl.cpp:730-1213), but one HIP stream per context, persistent scratch arenas instead of per-call cl buffers,
// and a device-resident layer (section 2 of the header) underneath the blocking host-pointer layer (section 1).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include "../../include/basisu_hip.h"
#include "tile_geometry_check.h"

// A grow-only device buffer: the per-call temporaries of the blocking layer live here so that repeated calls
// (one per frontend stage, several per refinement iteration) do not hit hipMalloc/hipFree.
struct arena {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = std::max(bytes, (size_t)4096);
        want += want / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct bu_hip_context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // a second stream for work that is independent of what the main stream is doing (the one-workgroup TSVQ splits of a round next to
    // its many-workgroup ones); joined back through the two events before anything reads the results
    hipStream_t side_stream = nullptr; hipEvent_t side_fork = nullptr, side_join = nullptr;
    bool dedicated_queue = false;         // own_stream was made with a (full) CU mask: a hardware queue of its own instead of a share of the runtime's pool
    // UASTC pipeline lanes with reserved walk CUs (bu_hip_tuning::uastc_walk_cus): the lean strip walk of uastc_rdo goes to walk_stream, whose CU mask is the reserved
    // set; own_stream (and with it everything that fills the chip) is masked to the OTHER CUs, side_stream (the walk with the refit in it) to the reserved ones
    hipStream_t walk_stream = nullptr; hipEvent_t walk_join = nullptr; uint32_t walk_cus = 0;
    arena refine_lists;                   // the sorted candidate lists of refine_endpoint_clusterization (etc1s_refine_kernels.hip, k_refine_sort_lists)
    arena etc1s_bc1_tables;               // the ETC1S -> BC1 endpoint tables (api_etc1s_transcode.cpp), built by the first BC1 transcode of the context
    arena etc1s_astc_tables;              // the two ETC1S -> ASTC look-ups and the unquantised endpoint values, built by the first ASTC transcode
    arena etc1s_atc_tables;               // the three ETC1S -> ATC / PVRTC2 look-ups 55, 56, 45, built by the first ATC RGB or PVRTC2 RGB / RGBA transcode
    arena etc1s_bc7_tables;               // the ETC1S -> BC7 colour look-up and the mode-5 encoder's midpoints, built by the first BC7 transcode
    const void* d_pixel_blocks = nullptr; // resident tiles (a1): 64 B per block
    size_t total_blocks = 0;
    arena pixel_arena;                    // owns the tiles when they were uploaded through bu_hip_set_pixel_blocks
    arena scratch[6];
    // pinned staging ring for host -> device uploads of pageable caller memory (h2d, api_context.cpp)
    void* stage = nullptr; size_t stage_cap = 0, stage_used = 0;
    void* bounce = nullptr; size_t bounce_cap = 0;   // pinned bounce buffer of device -> host downloads under a wait hook (bu_hip_memcpy_d2h)
    // small results (mail_fetch): a coherent page-locked buffer a one-workgroup kernel copies them into, followed by a word the host looks at; -1 = not available
    void* mail = nullptr; char* mail_dev = nullptr; int mail_state = 0; uint32_t mail_seq = 0;
    // pipelined tile upload (bu_hip_k_upload_and_encode_etc1s_blocks): a pinned ring of UP_SLOTS pieces the helper threads fill, one event per piece in flight
    void* up_ring = nullptr; size_t up_ring_cap = 0; std::vector<hipEvent_t> up_events;
    // background downloads (bu_hip_download_*): their own stream, so that a copy never sits in front of the side stream's kernels; events recycled; handles not yet waited for
    hipStream_t copy_stream = nullptr; std::vector<hipEvent_t> down_events;
    // ... carried out by ONE helper thread per context, started with the first download and parked on a condition variable between them (starting a thread per
    // download cost the calling thread 30-40 us each, on the step's critical path)
    std::thread down_thread; std::mutex down_mu; std::condition_variable down_cv, down_done_cv; std::deque<struct bu_hip_download*> down_queue; bool down_stop = false;
    std::string error;
    // bu_hip_malloc / bu_hip_free recycle blocks per context: an encoder frees and re-allocates the same dozen buffers for every
    // image, and hipMalloc/hipFree cost 0.1-1 ms each (hipFree also synchronises the device). Reuse is stream-ordered: everything
    // that touches these blocks is enqueued on the context's stream.
    void* tsvq_pinned = nullptr; size_t tsvq_pinned_cap = 0;  // recycled by bu_tsvq objects (one alive at a time per stream in practice)
    struct pooled { void* p; size_t cap; };
    std::vector<pooled> pool_free;
    std::vector<pooled> pool_live;
    size_t pool_free_bytes = 0;
    // optional per-kernel timing with HIP events on the launch stream (bu_hip_profile_*)
    int profiling = 0;   // bu_hip_profile_enable: 0 off, 1 every region, 2 the regions that are one kernel launch each
    struct prof_rec { const char* name; hipEvent_t start, stop; };
    std::vector<prof_rec> prof_pending;
    std::vector<hipEvent_t> prof_events;   // recycled (creating and destroying two events per timed region cost more host time than recording them)
    struct prof_sum { const char* name; double ms; uint32_t launches; };
    std::vector<prof_sum> prof_totals;
    bu_hip_tuning tuning{};               // bu_hip_set_tuning; starts as the process defaults (measured values, environment overrides read once)
    // cooperative waiting (bu_hip_set_wait_hook): called between looks at the stream wherever a call on this context would block its host thread
    bu_hip_wait_fn wait_hook = nullptr; void* wait_user = nullptr;
    // bu_hip_on_destroy registrations
    std::mutex closing_lock;
    std::vector<std::pair<bu_hip_destroy_fn, void*>> closing;
};

void set_error(bu_hip_context* ctx, const char* fmt, ...);   // ctx == nullptr: the process-wide error text
#define BU_TRY(ctx, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { set_error(ctx, "%s: %s", #expr, hipGetErrorString(e__)); return 0; } } while (0)

// defined, and described, in api_context.cpp
bu_hip_context* create_context_kind(int device, bool want_dedicated);
hipError_t stream_wait(bu_hip_context* ctx, hipStream_t s);
hipError_t d2h_pageable(bu_hip_context* ctx, void* h, const void* d, size_t bytes);
hipError_t h2d(bu_hip_context* ctx, void* d, const void* h, size_t bytes);
int wait_flag(bu_hip_context* ctx, int poll_mode, volatile uint32_t* round_flag, uint32_t seq, const char* label);
int fetch(bu_hip_context* ctx, void* h, const void* d, size_t bytes);
bool ensure_side_stream(bu_hip_context* ctx);
hipStream_t make_dedicated_stream(int device, uint32_t reserve = 0, bool reserved_side = false);
int quality_from_perms(uint32_t total_perms);
inline uint32_t next_seq(uint32_t& seq) { return ++seq ? seq : ++seq; }   // the next sequence number a kernel stores for wait_flag: never 0

// the reference's transcoder_texture_format names, for the refusals of the transcoders and the unpacker
inline const char* transcoder_format_name(uint32_t format) {
    static const char* const names[] = { "ETC1_RGB", "ETC2_RGBA", "BC1_RGB", "BC3_RGBA", "BC4_R", "BC5_RG", "BC7_RGBA", "BC7_ALT", "PVRTC1_4_RGB", "PVRTC1_4_RGBA", "ASTC_4x4_RGBA",
                                         "ATC_RGB", "ATC_RGBA", "RGBA32", "RGB565", "BGR565", "RGBA4444", "FXT1_RGB", "PVRTC2_4_RGB", "PVRTC2_4_RGBA", "ETC2_EAC_R11", "ETC2_EAC_RG11" };
    return format < sizeof(names) / sizeof(names[0]) ? names[format] : "unknown";
}

// A check of tile_geometry_check.h with its refusal as the context's error: checked(ctx, [&](bu::err_text e) { return bu::resolve_geometry(..., e); })
template <class Check>
inline int checked(bu_hip_context* ctx, Check check) {
    char text[512];
    if (check(bu::err_text{ text, sizeof(text) })) return 1;
    set_error(ctx, "%s", text);
    return 0;
}

// a small result copied back and waited for; not the mailbox path of fetch()
inline int read_back(bu_hip_context* ctx, void* h, const void* d, size_t bytes) {
    BU_TRY(ctx, d2h_pageable(ctx, h, d, bytes));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}

// A slice_table (tile_geometry_check.h) in scratch[4], sent in one stream-ordered copy: where its three parts are on the device. The counters, where the table has
// them, are not part of the copy: the launcher clears them.
struct uploaded_slices { const void* records; const uint32_t* prefix; uint32_t* counters; };
inline int upload_slice_table(bu_hip_context* ctx, const bu::slice_table& t, uploaded_slices& d) {
    arena& table = ctx->scratch[4];
    BU_TRY(ctx, table.reserve(t.pack.size()));
    BU_TRY(ctx, h2d(ctx, table.p, t.pack.data(), t.upload_bytes()));
    uint8_t* base = static_cast<uint8_t*>(table.p);
    d = uploaded_slices{ base, reinterpret_cast<const uint32_t*>(base + t.prefix_at), reinterpret_cast<uint32_t*>(base + t.counters_at) };
    return 1;
}
// every refusal the two whole-file transcoders share (api_transcode_slices.cpp): nothing is touched when it returns 0
int transcode_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target,
                           bool etc1s, const void* d_out, size_t out_bytes);
// the same for a UASTC table under the fourteen targets of bu_hip_k_transcode_uastc_textures
int uastc_texture_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs,
                               uint32_t target, const void* d_out, size_t out_bytes);
// the same for an ETC1S table under the target list of one of the ETC1S families: `unit` is what the family's unit function says of the target; two_wide: an output
// block covers two source blocks side by side (FXT1)
int etc1s_slices_check(bu_hip_context* ctx, bu::slice_table& t, const char* fn, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint64_t n_inputs, uint32_t target,
                       uint32_t unit, const void* d_out, size_t out_bytes, bool two_wide = false);

struct device_guard {
    int prev = -1; bool ok = false;
    explicit device_guard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
    }
    ~device_guard() { /* leave the context's device current: callers (torch) re-select theirs explicitly */ }
};

// RAII bracket around one kernel launch sequence: records a start/stop event pair on the launch stream when profiling is on.
struct prof_scope {
    bu_hip_context* ctx; const char* name; hipEvent_t start = nullptr, stop = nullptr;
    prof_scope(bu_hip_context* c, const char* n) : ctx(c), name(n) { if (ctx->profiling) begin(); }
    void begin();
    ~prof_scope() {
        if (!start) return;
        (void)hipEventRecord(stop, ctx->stream);
        ctx->prof_pending.push_back({name, start, stop});
    }
};

// Small device results for the host without a copy command (what that saves: at the definitions in api_context.cpp). Up to four parts per wait; what does not fit, or a context without the buffer, takes the copy.
struct mail_fetch {
    bu_hip_context* ctx;
    struct part { void* h; const void* d; size_t at, bytes; } parts[4];
    int n = 0; size_t used = 0; bool copied = false;
    explicit mail_fetch(bu_hip_context* c) : ctx(c) {}
    bool usable(); hipError_t add(void* h, const void* d, size_t bytes);
    int wait();   // 1 = everything added is in the caller's memory
};
