// api_context.cpp -- init / deinit, contexts (created, parked, destroyed), tuning, wait hook, block pool, copies, downloads, profiling; the helpers api_internal.h declares.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdlib>
#include "api_internal.h"
#include "etc1s_kernels.h"
#include "tsvq_kernels.h"
#include "tsvq_bufs.h"

// The process-wide state: defined here and nowhere else.
static std::mutex g_init_mutex;
static bool g_initialized = false;
static int g_device_count = 0;
static std::string g_global_error;
// contexts in use (handed out and not yet given back, so not parked): with more than one, a host thread that waits for its device round shares the cores with the others' host work
static std::atomic<int> g_live_contexts{0};
// Contexts are PARKED, not torn down, when they are destroyed: the reference's throughput driver (basis_parallel_compress, comp.cpp:5466-5559) creates one accelerator
// context per image and destroys it with the image, and a context's worth of device buffers costs ~20 hipMalloc calls to build and as many hipFree calls -- each one a
// DEVICE-wide synchronisation that stalls every other image's stream -- to tear down. A parked context keeps its stream, its workspaces and its block pool; the next
// bu_hip_create_context on that device gets it back, warm. At most BU_HIP_PARKED_CONTEXTS (default 16, 0 = off) are kept; bu_hip_deinit releases them.
static std::mutex g_park_lock;
static std::vector<bu_hip_context*> g_parked;

void set_error(bu_hip_context* ctx, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (ctx) ctx->error = buf; else g_global_error = buf;
}

// Every wait of a call for its context's own stream. Default: block the host thread. With a wait hook (a host that runs several contexts as cooperative tasks
// on one thread: bu_frontend_pipeline_*) the stream is only ever QUERIED and the hook runs between the looks -- it switches to another task and returns when it is
// this one's turn again.
hipError_t stream_wait(bu_hip_context* ctx, hipStream_t s) {
    if (!ctx->wait_hook) return hipStreamSynchronize(s);
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        ctx->wait_hook(ctx->wait_user);
    }
}

// Device -> host copy into PAGEABLE caller memory, enqueued on the context's stream. The runtime blocks the calling thread inside such a copy until the stream has
// drained; under a wait hook the draining is waited for cooperatively first, so that what blocks is only the (microseconds of a) copy from an idle stream.
hipError_t d2h_pageable(bu_hip_context* ctx, void* h, const void* d, size_t bytes) {
    if (ctx->wait_hook) { const hipError_t e = stream_wait(ctx, ctx->stream); if (e != hipSuccess) return e; }
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
}

// Waits for the word a one-thread kernel (k_tsvq_signal / the tail of k_mail_copy) stores into a coherent page-locked buffer. 1 = seen, 0 = the stream failed (error text set, under the caller's `label`).
int wait_flag(bu_hip_context* ctx, int poll_mode, volatile uint32_t* round_flag, uint32_t seq, const char* label) {
    // One context in the process: spin (the round trip is what the step waits for). Several (basis_parallel_compress, images in flight): the device is shared, a round
    // can take milliseconds, and a spinning waiter takes a core from another image's host backend -- after 30 us the core is offered to whoever wants it, after
    // 2 ms the thread sleeps between looks. bu_hip_tuning::tsvq_poll (BU_TSVQ_POLL=spin|yield) overrides.
    const bool polite = !ctx->wait_hook && (poll_mode == 2 || (poll_mode == 0 && g_live_contexts.load(std::memory_order_relaxed) > 1));
    const auto t_wait0 = std::chrono::steady_clock::now();
    auto last_query = t_wait0;
    for (;;) {
        if (*round_flag == seq) break;
        if (ctx->wait_hook) {   // cooperative: another task of this host thread runs while the round is on the device
            ctx->wait_hook(ctx->wait_user);
            if (*round_flag == seq) break;
        }
        const auto t_now = std::chrono::steady_clock::now();
        if (polite && t_now - t_wait0 > std::chrono::microseconds(30)) {
            if (t_now - t_wait0 > std::chrono::milliseconds(2)) std::this_thread::sleep_for(std::chrono::microseconds(50));
            else std::this_thread::yield();
        }
        if (t_now - last_query > std::chrono::microseconds(200)) {   // every 200 us: did the stream die, or finish without the flag becoming visible?
            last_query = t_now;
            const hipError_t e = hipStreamQuery(ctx->stream);
            if (e == hipSuccess) { __atomic_thread_fence(__ATOMIC_SEQ_CST); if (*round_flag != seq) BU_TRY(ctx, stream_wait(ctx, ctx->stream)); break; }
            if (e != hipErrorNotReady) { set_error(ctx, "%s: %s", label, hipGetErrorString(e)); return 0; }
        }
        __builtin_ia32_pause();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return 1;
}

// Small device results for the host WITHOUT a copy command: a one-workgroup kernel copies them into a coherent page-locked buffer and stores a sequence number behind them,
// the host looks at that word (wait_flag: spinning, yielding or running the wait hook) and copies them out. A hipMemcpyAsync into pageable memory + hipStreamSynchronize
// costs a blit launch by the runtime, its completion signal and the wake-up: 25-40 us between the producing kernel and the host's next launch; this is ~10.
// Up to four parts per wait (results that live in different arrays); what does not fit, or a context without the buffer, takes the copy.
constexpr size_t MAIL_BYTES = (size_t)64 << 10, MAIL_FLAG_AT = MAIL_BYTES;
bool mail_fetch::usable() {
    if (ctx->mail_state == 0) {
        ctx->mail_state = -1;
        static const bool on = [] { const char* e = std::getenv("BU_MAIL_FETCH"); return !e || e[0] != '0'; }();   // A/B switch
        if (!on) return false;
        void* p = nullptr;
        if (hipHostMalloc(&p, MAIL_BYTES + 256, hipHostMallocCoherent) == hipSuccess) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) { ctx->mail = p; ctx->mail_dev = static_cast<char*>(dp); ctx->mail_state = 1; *reinterpret_cast<volatile uint32_t*>(static_cast<char*>(p) + MAIL_FLAG_AT) = 0; }
            else { (void)hipGetLastError(); (void)hipHostFree(p); }
        } else (void)hipGetLastError();
    }
    return ctx->mail_state == 1;
}
hipError_t mail_fetch::add(void* h, const void* d, size_t bytes) {
    if (!bytes) return hipSuccess;
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (n == 4 || used + need > MAIL_BYTES || !usable()) { copied = true; return d2h_pageable(ctx, h, d, bytes); }
    parts[n++] = part{h, d, used, bytes};
    used += need;
    return hipSuccess;
}
int mail_fetch::wait() {
    if (n) {
        const uint32_t seq = next_seq(ctx->mail_seq);
        volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(static_cast<char*>(ctx->mail) + MAIL_FLAG_AT);
        for (int i = 0; i < n; i++)
            BU_TRY(ctx, bu::launch_mail_copy(ctx->stream, ctx->mail_dev + parts[i].at, parts[i].d, parts[i].bytes, i + 1 == n ? reinterpret_cast<uint32_t*>(ctx->mail_dev + MAIL_FLAG_AT) : nullptr, seq));
        if (!wait_flag(ctx, (int)ctx->tuning.tsvq_poll, flag, seq, "mail_fetch")) return 0;
        for (int i = 0; i < n; i++) std::memcpy(parts[i].h, static_cast<const char*>(ctx->mail) + parts[i].at, parts[i].bytes);
    }
    if (copied || !n) BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}
// device -> host + wait, one result
int fetch(bu_hip_context* ctx, void* h, const void* d, size_t bytes) {
    mail_fetch f(ctx);
    BU_TRY(ctx, f.add(h, d, bytes));
    return f.wait();
}

static void prof_add(bu_hip_context* ctx, const bu_hip_context::prof_rec& r) {   // a finished region's time onto its name's total
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, r.start, r.stop) != hipSuccess) return;
    for (auto& t : ctx->prof_totals) if (t.name == r.name) { t.ms += ms; t.launches++; return; }
    ctx->prof_totals.push_back({r.name, (double)ms, 1u});
}

void prof_scope::begin() {   // profiling is on: take (recycled) events and record the start
    // level 2: only the regions that are ONE kernel launch; the many-launch regions (codebook builders' rounds, de-duplication sorts, list bookkeeping) go untimed,
    // and with them the events that would sit between their kernels
    if (ctx->profiling == 2 && (std::strncmp(name, "tsvq_", 5) == 0 || std::strncmp(name, "unique_", 7) == 0 || std::strncmp(name, "map_", 4) == 0 || std::strncmp(name, "kmeans_", 7) == 0)) return;
    if (ctx->prof_events.size() < 2 && ctx->prof_pending.size() >= 64) {   // reap the oldest finished regions: their events are the next ones recorded
        size_t done = 0;
        while (done < ctx->prof_pending.size() && done < 8 && hipEventQuery(ctx->prof_pending[done].stop) == hipSuccess) {
            const bu_hip_context::prof_rec& r = ctx->prof_pending[done++];
            prof_add(ctx, r);
            ctx->prof_events.push_back(r.start); ctx->prof_events.push_back(r.stop);
        }
        if (done) ctx->prof_pending.erase(ctx->prof_pending.begin(), ctx->prof_pending.begin() + (long)done);
        (void)hipGetLastError();   // a hipErrorNotReady of the last look must not be what the next launcher's hipGetLastError() finds
    }
    auto take = [&](hipEvent_t& e) {
        if (!ctx->prof_events.empty()) { e = ctx->prof_events.back(); ctx->prof_events.pop_back(); return true; }
        return hipEventCreate(&e) == hipSuccess;
    };
    if (!take(start)) { start = nullptr; return; }
    if (!take(stop)) { ctx->prof_events.push_back(start); start = stop = nullptr; return; }
    (void)hipEventRecord(start, ctx->stream);
}

static void prof_drain(bu_hip_context* ctx) {
    for (auto& r : ctx->prof_pending) {
        if (hipEventSynchronize(r.stop) == hipSuccess) prof_add(ctx, r);
        ctx->prof_events.push_back(r.start); ctx->prof_events.push_back(r.stop);
    }
    ctx->prof_pending.clear();
}

// Host -> device upload of caller-owned (pageable) memory, ordered on the context's stream. Pageable memory is never handed to
// hipMemcpyAsync: on this stack (ROCm 7.2, MI355X) a kernel launched right behind such a copy was observed to read the
// destination before the data had landed (tools/tsvq_root_repeat.py). Small uploads go through a pinned staging ring (a real
// stream-ordered DMA; the ring is recycled only after a stream synchronise), large ones through a blocking hipMemcpy.
hipError_t h2d(bu_hip_context* ctx, void* d, const void* h, size_t bytes) {
    if (!bytes) return hipSuccess;
    hipError_t e;
    if (bytes > ((size_t)4 << 20)) {
        // large uploads (an image's tiles) go through the ring in 4 MiB pieces: a blocking hipMemcpy + hipDeviceSynchronize here made every image's upload wait for
        // every OTHER context's kernels (basis_parallel_compress: one context per image in flight), which serialised the images
        for (size_t at = 0; at < bytes; at += (size_t)4 << 20) {
            const size_t piece = std::min(bytes - at, (size_t)4 << 20);
            if ((e = h2d(ctx, static_cast<char*>(d) + at, static_cast<const char*>(h) + at, piece)) != hipSuccess) return e;
        }
        return hipSuccess;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (need > ctx->stage_cap - ctx->stage_used) {
        if ((e = stream_wait(ctx, ctx->stream)) != hipSuccess) return e; // every copy out of the ring has completed
        ctx->stage_used = 0;
        if (need > ctx->stage_cap) {
            if (ctx->stage) { (void)hipHostFree(ctx->stage); ctx->stage = nullptr; ctx->stage_cap = 0; }
            const size_t want = std::max(need * 2, (size_t)16 << 20);
            if ((e = hipHostMalloc(&ctx->stage, want, hipHostMallocDefault)) != hipSuccess) { ctx->stage = nullptr; return e; }
            ctx->stage_cap = want;
        }
    }
    char* slot = static_cast<char*>(ctx->stage) + ctx->stage_used;
    std::memcpy(slot, h, bytes);
    ctx->stage_used += need;
    return hipMemcpyAsync(d, slot, bytes, hipMemcpyHostToDevice, ctx->stream);
}

int quality_from_perms(uint32_t total_perms) {
    // frontend.cpp:746-752 / etc.cpp:792-800: {4,16,64,165} <-> {fast, medium, slow, uber}
    if (total_perms <= 4) return bu::BU_Q_FAST;
    if (total_perms <= 16) return bu::BU_Q_MEDIUM;
    if (total_perms <= 64) return bu::BU_Q_SLOW;
    return bu::BU_Q_UBER;
}

// A stream with a hardware queue of its own: hipExtStreamCreateWithCUMask with every CU enabled (the runtime does not pool queues that carry a CU mask). nullptr on failure.
// reserve = 0: every CU. Otherwise the device's CUs are split into a RESERVED set of about `reserve` CUs -- every (CUs / reserve)-th one, so that whatever order the
// mask's bits have over XCDs and shader engines, every one of them gives its share -- and the rest; reserved_side picks which of the two the stream may use.
hipStream_t make_dedicated_stream(int device, uint32_t reserve, bool reserved_side) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || prop.multiProcessorCount <= 0) { (void)hipGetLastError(); return nullptr; }
    const uint32_t cus = (uint32_t)prop.multiProcessorCount;
    std::vector<uint32_t> mask((cus + 31) / 32, 0xFFFFFFFFu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    if (reserve && reserve < cus) {
        const uint32_t stride = cus / reserve;
        for (uint32_t i = 0; i < cus; i++) {
            const bool is_reserved = stride >= 2 ? (i % stride == stride - 1) : (i < reserve);
            if (is_reserved != reserved_side) mask[i / 32] &= ~(1u << (i % 32));
        }
    }
    hipStream_t s = nullptr;
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return s;
}

// The context's second stream (and the two events that fork it off the main stream and join it back), made on first use.
bool ensure_side_stream(bu_hip_context* ctx) {
    if (ctx->side_stream) return true;
    if (hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess || (!ctx->side_fork && hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming) != hipSuccess) ||
        (!ctx->side_join && hipEventCreateWithFlags(&ctx->side_join, hipEventDisableTiming) != hipSuccess)) {
        (void)hipGetLastError();
        if (ctx->side_stream) { (void)hipStreamDestroy(ctx->side_stream); ctx->side_stream = nullptr; }
        if (ctx->side_fork) { (void)hipEventDestroy(ctx->side_fork); ctx->side_fork = nullptr; }
        if (ctx->side_join) { (void)hipEventDestroy(ctx->side_join); ctx->side_join = nullptr; }
        return false;
    }
    return true;
}

static size_t park_limit() {
    static const size_t n = [] { const char* e = std::getenv("BU_HIP_PARKED_CONTEXTS"); const long v = e ? std::atol(e) : 16; return (size_t)(v < 0 ? 0 : (v > 64 ? 64 : v)); }();
    return n;
}

// The process defaults of bu_hip_tuning: measured values, each overridable ONCE per process by the environment variable named in basisu_hip.h.
static const bu_hip_tuning& default_tuning() {
    static const bu_hip_tuning t = [] {
        bu_hip_tuning d;
        std::memset(&d, 0, sizeof(d));
        d.struct_bytes = (uint32_t)sizeof(d);
        d.tsvq_wide_min = 8192; d.tsvq_wide6_min = 8192; d.tsvq_wide_cov_min = 98304; d.tsvq_windows = 0; d.tsvq_dense_min = 257; d.tsvq_zero_copy = 1; d.tsvq_deep_levels = 0; d.uastc_walk_cus = 0; d.codebook_wide_min = 32768;
        auto num = [](const char* name, long lo, long hi, uint32_t* out) { if (const char* e = std::getenv(name)) { const long v = std::atol(e); if (v >= lo && v <= hi) *out = (uint32_t)v; } };
        num("BU_TSVQ_WIDE_MIN", 512, 1l << 30, &d.tsvq_wide_min);
        num("BU_TSVQ_WIDE6_MIN", 512, 1l << 30, &d.tsvq_wide6_min);
        num("BU_TSVQ_WIDE_COV_MIN", 0, 1l << 30, &d.tsvq_wide_cov_min);
        num("BU_TSVQ_DENSE_MIN", 0, 1l << 30, &d.tsvq_dense_min);
        num("BU_TSVQ_ZEROCOPY", 0, 1, &d.tsvq_zero_copy);
        num("BU_TSVQ_DEEP", 0, (long)bu::TSVQ_MAX_DEEP_LEVELS, &d.tsvq_deep_levels);
        num("BU_UASTC_WALK_CUS", 0, 128, &d.uastc_walk_cus);
        num("BU_CODEBOOK_WIDE_MIN", 0, 1l << 30, &d.codebook_wide_min);
        if (const char* e = std::getenv("BU_TSVQ_WIDE")) if (std::atoi(e) == 0) d.tsvq_wide_min = d.tsvq_wide6_min = 0;
        if (const char* e = std::getenv("BU_TSVQ_WIDE6")) if (std::atoi(e) == 0) d.tsvq_wide6_min = 0;
        if (const char* e = std::getenv("BU_TSVQ_WINDOWS")) d.tsvq_windows = e[0] == '0' ? 2u : 1u;
        if (std::getenv("BU_TSVQ_CHAINED")) d.tsvq_chained_only = 1;
        if (const char* e = std::getenv("BU_TSVQ_POLL")) d.tsvq_poll = e[0] == 's' ? 1u : 2u;
        d.debug = (std::getenv("BU_TSVQ_ROUNDS") ? 1u : 0u) | (std::getenv("BU_TSVQ_SERIAL") ? 2u : 0u) | (std::getenv("BU_TSVQ_STATS") ? 4u : 0u);
        return d;
    }();
    return t;
}

// A parked context keeps its stream, and with it the KIND of queue the stream sits on: the lanes of a UASTC pipeline run on hardware queues of their own (dedicated_queue),
// everybody else on the runtime's pooled ones -- ETC1S frontend jobs measured 15-20 % slower with every context on its own queue. So a caller gets a parked context of
// the kind it asks for: the public create calls never a dedicated-queue one, the UASTC pipeline those first.
bu_hip_context* create_context_kind(int device, bool want_dedicated) {
    if (!g_initialized) { set_error(nullptr, "bu_hip_create_context: bu_hip_init() has not succeeded"); return nullptr; }
    if (device < 0 || device >= g_device_count) { set_error(nullptr, "bu_hip_create_context: bad device %d", device); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_error(nullptr, "hipSetDevice(%d) failed", device); return nullptr; }
    {
        std::lock_guard<std::mutex> g(g_park_lock);
        for (int pass = 0; pass < (want_dedicated ? 2 : 1); pass++)   // (a lane that finds no parked context of its own kind takes a pooled one and moves it onto a queue of its own)
            for (size_t i = 0; i < g_parked.size(); i++)
                if (g_parked[i]->device == device && g_parked[i]->dedicated_queue == (want_dedicated && pass == 0)) {
                    bu_hip_context* c = g_parked[i]; g_parked.erase(g_parked.begin() + (long)i); g_live_contexts.fetch_add(1); return c;
                }
    }
    bu_hip_context* ctx = new (std::nothrow) bu_hip_context();
    if (!ctx) return nullptr;
    ctx->device = device;
    ctx->tuning = default_tuning();
    // (a pooled queue, not a dedicated one: with EVERY context on a queue of its own the frontend pipeline lost 15-20 %, measured)
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { set_error(nullptr, "hipStreamCreate failed"); delete ctx; return nullptr; }
    ctx->stream = ctx->own_stream;
    hipError_t e = bu::upload_block_fit_tables();
    if (e == hipSuccess) e = bu::upload_cluster_fit_tables();
    if (e != hipSuccess) { set_error(nullptr, "constant table upload failed: %s", hipGetErrorString(e)); (void)hipStreamDestroy(ctx->own_stream); delete ctx; return nullptr; }
    g_live_contexts.fetch_add(1);
    return ctx;
}

static void context_release(bu_hip_context* ctx) {   // the real teardown
    (void)hipSetDevice(ctx->device);
    ctx->pixel_arena.release();
    for (auto& a : ctx->scratch) a.release();
    ctx->refine_lists.release();
    ctx->etc1s_bc1_tables.release();
    ctx->etc1s_bc7_tables.release();
    ctx->etc1s_astc_tables.release();
    ctx->etc1s_atc_tables.release();
    if (ctx->tsvq_pinned) (void)hipHostFree(ctx->tsvq_pinned);
    for (auto& b : ctx->pool_free) (void)hipFree(b.p);
    for (auto& b : ctx->pool_live) (void)hipFree(b.p);
    if (ctx->stage) (void)hipHostFree(ctx->stage);
    if (ctx->bounce) (void)hipHostFree(ctx->bounce);
    if (ctx->mail) (void)hipHostFree(ctx->mail);
    if (ctx->up_ring) (void)hipHostFree(ctx->up_ring);
    if (ctx->down_thread.joinable()) {
        { std::lock_guard<std::mutex> lk(ctx->down_mu); ctx->down_stop = true; }
        ctx->down_cv.notify_all();
        ctx->down_thread.join();
    }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (hipEvent_t e : ctx->down_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->up_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
    if (ctx->walk_stream) (void)hipStreamDestroy(ctx->walk_stream);
    if (ctx->walk_join) (void)hipEventDestroy(ctx->walk_join);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->side_fork) (void)hipEventDestroy(ctx->side_fork);
    if (ctx->side_join) (void)hipEventDestroy(ctx->side_join);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" {
// ---------------------------------------------------------------------------------------------------------------- init

int bu_hip_init(int /*force_serialization*/) {
    // (No environment is touched here. Streams of a process share a few hardware queues -- GPU_MAX_HW_QUEUES, ROCm's default: 4 -- and two streams that land on one
    // queue run their kernels one after the other; a host that wants more than four lanes side by side sets that variable itself before its first HIP call: INTEGRATION.md.)
    std::lock_guard<std::mutex> lock(g_init_mutex);
    if (g_initialized) return 1;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(nullptr, "bu_hip_init: no HIP device (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e));
        (void)hipGetLastError();
        return 0;
    }
    g_device_count = n;
    g_initialized = true;
    return 1;
}

void bu_hip_deinit(void) {
    std::vector<bu_hip_context*> parked;
    { std::lock_guard<std::mutex> g(g_park_lock); parked.swap(g_parked); }
    for (bu_hip_context* c : parked) context_release(c);
    std::lock_guard<std::mutex> lock(g_init_mutex);
    g_initialized = false;
}

int bu_hip_is_available(void) { return g_initialized ? 1 : 0; }

bu_hip_context* bu_hip_create_context_on(int device) { return create_context_kind(device, false); }

bu_hip_context* bu_hip_create_context(void) {
    int dev = 0;
    if (!g_initialized) { set_error(nullptr, "bu_hip_create_context: bu_hip_init() has not succeeded"); return nullptr; }
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return bu_hip_create_context_on(dev);
}

int bu_hip_on_destroy(bu_hip_context* ctx, bu_hip_destroy_fn fn, void* user) {
    if (!ctx || !fn) return 0;
    std::lock_guard<std::mutex> g(ctx->closing_lock);
    ctx->closing.emplace_back(fn, user);
    return 1;
}
void bu_hip_cancel_on_destroy(bu_hip_context* ctx, bu_hip_destroy_fn fn, void* user) {
    if (!ctx) return;
    std::lock_guard<std::mutex> g(ctx->closing_lock);
    for (size_t i = 0; i < ctx->closing.size(); i++)
        if (ctx->closing[i].first == fn && ctx->closing[i].second == user) { ctx->closing.erase(ctx->closing.begin() + (long)i); break; }
}

void bu_hip_destroy_context(bu_hip_context* ctx) {
    if (!ctx) return;
    g_live_contexts.fetch_sub(1);
    (void)hipSetDevice(ctx->device);
    for (;;) {  // dependents first (a callback may cancel others; each runs once, outside the lock)
        std::pair<bu_hip_destroy_fn, void*> cb;
        {
            std::lock_guard<std::mutex> g(ctx->closing_lock);
            if (ctx->closing.empty()) break;
            cb = ctx->closing.back(); ctx->closing.pop_back();
        }
        cb.first(cb.second);
    }
    bool healthy = stream_wait(ctx, ctx->stream) == hipSuccess;
    if (ctx->side_stream) healthy = hipStreamSynchronize(ctx->side_stream) == hipSuccess && healthy;
    if (ctx->own_stream != ctx->stream) healthy = hipStreamSynchronize(ctx->own_stream) == hipSuccess && healthy;
    if (!healthy) (void)hipGetLastError();
    prof_drain(ctx);
    if (park_limit() && healthy) {   // a context whose streams ended in an error is torn down, never handed to the next creator
        // back to the state bu_hip_create_context_on hands out, with the memory kept: blocks the caller leaked join the free list (the context owns all device memory it handed out)
        for (auto& b : ctx->pool_live) { ctx->pool_free.push_back(b); ctx->pool_free_bytes += b.cap; }
        ctx->pool_live.clear();
        ctx->stream = ctx->own_stream;
        ctx->d_pixel_blocks = nullptr; ctx->total_blocks = 0;
        ctx->stage_used = 0;
        ctx->error.clear();
        ctx->profiling = 0; ctx->prof_totals.clear();
        ctx->wait_hook = nullptr; ctx->wait_user = nullptr;
        ctx->tuning = default_tuning();
        std::lock_guard<std::mutex> g(g_park_lock);
        if (g_parked.size() < park_limit()) { g_parked.push_back(ctx); return; }
    }
    context_release(ctx);
}

int bu_hip_context_device(const bu_hip_context* ctx) { return ctx ? ctx->device : -1; }
int bu_hip_set_stream(bu_hip_context* ctx, void* s) {
    if (!ctx) return 0;
    (void)stream_wait(ctx, ctx->stream); // staged uploads still in flight belong to the old stream
    ctx->stage_used = 0;
    ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
    return 1;
}
void* bu_hip_get_stream(bu_hip_context* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
const char* bu_hip_last_error(const bu_hip_context* ctx) { return ctx ? ctx->error.c_str() : g_global_error.c_str(); }
void bu_hip_set_last_error(bu_hip_context* ctx, const char* text) { set_error(ctx, "%s", text ? text : ""); }

void bu_hip_get_tuning(const bu_hip_context* ctx, bu_hip_tuning* out, uint32_t struct_bytes) {
    if (!out || struct_bytes < 8) return;
    const bu_hip_tuning& t = ctx ? ctx->tuning : default_tuning();
    std::memcpy(out, &t, std::min<size_t>(struct_bytes, sizeof(t)));
    out->struct_bytes = (uint32_t)std::min<size_t>(struct_bytes, sizeof(t));
}

int bu_hip_set_tuning(bu_hip_context* ctx, const bu_hip_tuning* t) {
    if (!ctx) return 0;
    if (!t) { ctx->tuning = default_tuning(); return 1; }
    if (t->struct_bytes < 8 || t->struct_bytes > 4096) { set_error(ctx, "bu_hip_set_tuning: struct_bytes %u", t->struct_bytes); return 0; }
    bu_hip_tuning n = default_tuning();   // fields a caller's older header does not have keep their defaults
    std::memcpy(&n, t, std::min<size_t>(t->struct_bytes, sizeof(n)));
    n.struct_bytes = (uint32_t)sizeof(n);
    if ((n.tsvq_wide_min && n.tsvq_wide_min < 512) || (n.tsvq_wide6_min && n.tsvq_wide6_min < 512) || n.tsvq_windows > 2 || n.tsvq_poll > 2 || n.refine_unsorted > 2 || n.tsvq_deep_levels > bu::TSVQ_MAX_DEEP_LEVELS) {
        set_error(ctx, "bu_hip_set_tuning: value out of range (many-workgroup thresholds are 0 or >= 512, windows / poll / refine_unsorted 0..2, deep levels 0..2)");
        return 0;
    }
    ctx->tuning = n;
    return 1;
}

int bu_hip_set_wait_hook(bu_hip_context* ctx, bu_hip_wait_fn fn, void* user) {
    if (!ctx) return 0;
    ctx->wait_hook = fn; ctx->wait_user = fn ? user : nullptr;
    return 1;
}

int bu_hip_sync(bu_hip_context* ctx) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}

void* bu_hip_malloc(bu_hip_context* ctx, size_t bytes) {
    if (!ctx) return nullptr;
    device_guard g(ctx->device);
    const size_t want = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
    // best fit among the cached blocks, but never more than twice (+1 MiB) what was asked for
    int best = -1;
    for (size_t i = 0; i < ctx->pool_free.size(); i++) {
        const size_t cap = ctx->pool_free[i].cap;
        if (cap >= want && cap <= want * 2 + ((size_t)1 << 20) && (best < 0 || cap < ctx->pool_free[(size_t)best].cap)) best = (int)i;
    }
    if (best >= 0) {
        const bu_hip_context::pooled b = ctx->pool_free[(size_t)best];
        ctx->pool_free.erase(ctx->pool_free.begin() + best);
        ctx->pool_free_bytes -= b.cap;
        ctx->pool_live.push_back(b);
        return b.p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        // out of memory: drop the cache and retry once
        (void)stream_wait(ctx, ctx->stream);
        for (auto& b : ctx->pool_free) (void)hipFree(b.p);
        ctx->pool_free.clear(); ctx->pool_free_bytes = 0;
        if (hipMalloc(&p, want) != hipSuccess) { set_error(ctx, "hipMalloc(%zu) failed", bytes); (void)hipGetLastError(); return nullptr; }
    }
    ctx->pool_live.push_back({p, want});
    return p;
}
void bu_hip_free(bu_hip_context* ctx, void* p) {
    if (!ctx || !p) return;
    device_guard g(ctx->device);
    for (size_t i = 0; i < ctx->pool_live.size(); i++)
        if (ctx->pool_live[i].p == p) {
            const bu_hip_context::pooled b = ctx->pool_live[i];
            ctx->pool_live.erase(ctx->pool_live.begin() + (long)i);
            if (ctx->pool_free_bytes + b.cap <= ((size_t)16 << 30)) { ctx->pool_free.push_back(b); ctx->pool_free_bytes += b.cap; return; }
            (void)stream_wait(ctx, ctx->stream);
            (void)hipFree(p);
            return;
        }
    // not a live block of this context: a second free of a pooled block (it is in pool_free and will be handed out again -- hipFree here would
    // turn that into a use after free) or a foreign pointer. Leave it alone and say so.
    set_error(ctx, "bu_hip_free: %p is not a live allocation of this context (double free?)", p);
}
int bu_hip_memcpy_h2d(bu_hip_context* ctx, void* d, const void* h, size_t bytes) {
    if (!ctx) return 0;
    if (!bytes) return 1;
    device_guard g(ctx->device);
    BU_TRY(ctx, h2d(ctx, d, h, bytes));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream)); // h may be pageable and released by the caller right after
    return 1;
}
// the same, stream-ordered: on return `h` has been copied out (into the context's pinned ring) and may be released; the device side is ordered with everything enqueued on
// the context's stream before and after. No host synchronisation (the ring synchronises the stream only when it wraps).
int bu_hip_memcpy_h2d_async(bu_hip_context* ctx, void* d, const void* h, size_t bytes) {
    if (!ctx) return 0;
    if (!bytes) return 1;
    device_guard g(ctx->device);
    BU_TRY(ctx, h2d(ctx, d, h, bytes));
    return 1;
}
int bu_hip_memcpy_d2h(bu_hip_context* ctx, void* h, const void* d, size_t bytes) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    if (ctx->wait_hook && bytes > 4096) {
        // cooperative host: hipMemcpyAsync into pageable memory would block this thread for the whole transfer (the runtime stages it synchronously). Through a pinned
        // bounce buffer the transfer is a real stream-ordered DMA and the thread's other tasks run while it is in flight.
        const size_t piece_max = (size_t)32 << 20;
        const size_t want = std::min(bytes, piece_max);
        if (want > ctx->bounce_cap) {
            if (ctx->bounce) { (void)hipHostFree(ctx->bounce); ctx->bounce = nullptr; ctx->bounce_cap = 0; }
            BU_TRY(ctx, hipHostMalloc(&ctx->bounce, want, hipHostMallocDefault));
            ctx->bounce_cap = want;
        }
        for (size_t at = 0; at < bytes; at += piece_max) {
            const size_t piece = std::min(bytes - at, piece_max);
            BU_TRY(ctx, hipMemcpyAsync(ctx->bounce, static_cast<const char*>(d) + at, piece, hipMemcpyDeviceToHost, ctx->stream));
            BU_TRY(ctx, stream_wait(ctx, ctx->stream));
            std::memcpy(static_cast<char*>(h) + at, ctx->bounce, piece);
        }
        return 1;
    }
    // small results travel without a copy command (mail_fetch); the rest: (under a wait hook the stream is drained cooperatively first: the runtime would block in the copy until it has)
    return fetch(ctx, h, d, bytes);
}
void* bu_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void bu_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- background downloads
struct bu_hip_download {
    bu_hip_context* ctx; hipEvent_t ready; void* h; const void* d; size_t bytes; bool done; hipError_t result;
};
static void download_worker(bu_hip_context* c) {
    (void)hipSetDevice(c->device);
    for (;;) {
        bu_hip_download* dl = nullptr;
        {
            std::unique_lock<std::mutex> lk(c->down_mu);
            c->down_cv.wait(lk, [&] { return c->down_stop || !c->down_queue.empty(); });
            if (c->down_queue.empty()) return;   // stop, and nothing left to do
            dl = c->down_queue.front(); c->down_queue.pop_front();
        }
        // this thread is what blocks in the copy (into pageable memory the runtime holds the calling thread for the whole transfer); the copy waits for `ready` on the device
        hipError_t e = hipStreamWaitEvent(c->copy_stream, dl->ready, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(dl->h, dl->d, dl->bytes, hipMemcpyDeviceToHost, c->copy_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->copy_stream);
        { std::lock_guard<std::mutex> lk(c->down_mu); dl->result = e; dl->done = true; }
        c->down_done_cv.notify_all();
    }
}
bu_hip_download* bu_hip_download_begin(bu_hip_context* ctx, void* h, const void* d, size_t bytes) {
    if (!ctx || !h || !d || !bytes || ctx->wait_hook) return nullptr;
    device_guard g(ctx->device);
    if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->copy_stream = nullptr; return nullptr; }
    if (!ctx->down_thread.joinable()) {
        try { ctx->down_thread = std::thread(download_worker, ctx); } catch (...) { return nullptr; }
    }
    hipEvent_t ev = nullptr;
    if (!ctx->down_events.empty()) { ev = ctx->down_events.back(); ctx->down_events.pop_back(); }
    else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipEventRecord(ev, ctx->stream) != hipSuccess) { (void)hipGetLastError(); ctx->down_events.push_back(ev); return nullptr; }
    bu_hip_download* dl = new (std::nothrow) bu_hip_download{ctx, ev, h, d, bytes, false, hipSuccess};
    if (!dl) { ctx->down_events.push_back(ev); return nullptr; }
    { std::lock_guard<std::mutex> lk(ctx->down_mu); ctx->down_queue.push_back(dl); }
    ctx->down_cv.notify_one();
    return dl;
}
int bu_hip_download_wait(bu_hip_download* dl) {
    if (!dl) return 0;
    bu_hip_context* ctx = dl->ctx;
    { std::unique_lock<std::mutex> lk(ctx->down_mu); ctx->down_done_cv.wait(lk, [&] { return dl->done; }); }
    ctx->down_events.push_back(dl->ready);
    const hipError_t e = dl->result;
    delete dl;
    if (e != hipSuccess) { set_error(ctx, "bu_hip_download: %s", hipGetErrorString(e)); (void)hipGetLastError(); return 0; }
    return 1;
}

int bu_hip_memcpy_d2d(bu_hip_context* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return 0;
    if (!bytes) return 1;
    device_guard g(ctx->device);
    BU_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 1;
}
int bu_hip_memset(bu_hip_context* ctx, void* d, int value, size_t bytes) {
    if (!ctx) return 0;
    if (!bytes) return 1;
    device_guard g(ctx->device);
    BU_TRY(ctx, hipMemsetAsync(d, value, bytes, ctx->stream));
    return 1;
}

int bu_hip_profile_enable(bu_hip_context* ctx, int on) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_drain(ctx);
    ctx->prof_totals.clear();
    ctx->profiling = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return 1;
}

uint32_t bu_hip_profile_read(bu_hip_context* ctx, const char** names, double* total_ms, uint32_t* launches, uint32_t cap) {
    if (!ctx) return 0;
    device_guard g(ctx->device);
    prof_drain(ctx);
    const uint32_t n = (uint32_t)std::min<size_t>(ctx->prof_totals.size(), cap);
    for (uint32_t i = 0; i < n; i++) { names[i] = ctx->prof_totals[i].name; total_ms[i] = ctx->prof_totals[i].ms; launches[i] = ctx->prof_totals[i].launches; }
    return (uint32_t)ctx->prof_totals.size();
}
} // extern "C"
