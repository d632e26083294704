// api_tsvq.cpp -- TSVQ behind the C ABI of libbasisu_hip.so (row a8): the host driver of the tree builds -- root, rounds of splits, span roots, spans, multi-GPU exchange.
#include <chrono>
#include "api_internal.h"
#include "tsvq_kernels.h"
#include "tsvq_bufs.h"
#include "bookkeeping_kernels.h"

struct bu_tsvq {
    uint32_t dim = 0, n = 0;
    bool packed = false;
    void* rows = nullptr;       // float[n][dim], or uint32[n] when packed
    uint64_t* w64 = nullptr;
    uint32_t* perm[2] = {nullptr, nullptr};   // perm[0]: ONE block of TSVQ_BUFS buffers of n indices each, perm[1] = perm[0] + n (tsvq_bufs.h: the pair gives every kernel base and stride)
    uint8_t* side = nullptr;
    arena nodes, outs;
    arena deep_nodes;           // deep rounds: the node records of generations 1.. (made on the device by k_tsvq_children)
    // the knobs below are copies of the context's bu_hip_tuning at creation (basisu_hip.h): one tree never changes paths half way
    bool force_chained = false; // tsvq_chained_only: never use the exact (integer-reduced) kernel variants (tests compare both)
    // Nodes with at least wide_min members go through the many-workgroup path (tsvq_wide_kernels.hip for packed rows, tsvq_wide6_kernels.hip for 6-float rows).
    uint32_t wide_min = 0;      // 0: off
    uint32_t wide_cov_min = 0;  // batches whose largest node is smaller run the covariance pass chained (tsvq_wide_cov_min)
    int windows = 0; uint32_t dense_min = 257; int poll = 0;
    uint32_t wide_blocks_cap = 0, wide_nodes_cap = 0;
    void* xchg = nullptr; size_t xchg_cap = 0;   // staging of bu_hip_tsvq_exchange_* (multi-GPU)
    void* wide_ws = nullptr; void* wide_packed = nullptr; bu::tsvq_wide_node* wide_nodes = nullptr; bu::tsvq_wide_ctrl* wide_ctrl = nullptr; void* wide_ctrl_raw = nullptr;
    // Pinned staging for the per-round node / result records: hipMemcpyAsync on PAGEABLE host memory followed directly by a
    // kernel on the same stream was observed to let the kernel read the destination before the copy landed (MI355X, ROCm 7.2:
    // tools/tsvq_root_repeat.py, 2 of 10 runs), so nothing on this path hands pageable memory to an asynchronous copy.
    void* pinned = nullptr; size_t pinned_cap = 0;
    // Zero-copy rounds (default; tsvq_zero_copy = 0 switches back to staged copies + hipStreamSynchronize): the one-workgroup kernel reads its node records
    // from, and every split kernel writes its result records to, the page-locked buffer directly; a one-thread kernel behind them raises `round_flag`
    // (system scope) and the host spins on it. That takes two copy launches and a blocking synchronisation out of every round of the tree build.
    bool zero_copy = true;
    uint32_t round_seq = 0;
    bool dbg_rounds = false, dbg_serial = false, dbg_stats = false;   // bu_hip_tuning::debug bits
    hipError_t reserve_pinned(size_t bytes) {
        if (bytes <= pinned_cap) return hipSuccess;
        if (pinned) { (void)hipHostFree(pinned); pinned = nullptr; pinned_cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        // coherent (fine-grained) host memory: the zero-copy rounds have kernels write result records and the completion word straight into this buffer while the host polls
        // it; with a non-coherent mapping the word would only become visible when the kernel retires
        hipError_t e = hipHostMalloc(&pinned, want, hipHostMallocCoherent);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostMalloc(&pinned, want, hipHostMallocDefault); zero_copy = false; }
        if (e != hipSuccess) { pinned = nullptr; return e; }
        pinned_cap = want;
        return hipSuccess;
    }
    hipError_t launch_split(hipStream_t st, bool exact, const bu::tsvq_node_in* d_nodes, uint32_t count, bu::tsvq_split_out* d_outs) const {   // the one-workgroup split kernel
        return bu::launch_tsvq_split(st, (int)dim, packed, exact, rows, w64, perm[0], perm[1], side, d_nodes, count, d_outs, dense_min);
    }
};

static_assert(sizeof(bu_tsvq_root) == sizeof(bu::tsvq_root_out), "layout");
static_assert(sizeof(bu_tsvq_node) == sizeof(bu::tsvq_node_in), "layout");
static_assert(sizeof(bu_tsvq_split) == sizeof(bu::tsvq_split_out), "layout");

// The buffers of the many-workgroup path for nodes of at least `wide_min` members (0, or fewer rows than that: off). member_bytes: of wide_packed. false = allocation failed.
static bool tsvq_alloc_wide(bu_hip_context* ctx, bu_tsvq* q, uint32_t wide_min, size_t member_bytes, uint32_t wide_cov_min) {
    const uint32_t n = q->n;
    if (!wide_min || n < wide_min || n >= (1u << 22)) return true;   // above 2^22 members the binade prediction loses its margin; the chained kernel takes those
    q->wide_min = wide_min; q->wide_cov_min = wide_cov_min;
    q->wide_nodes_cap = n / wide_min + 1; q->wide_blocks_cap = (n + 255) / 256 + q->wide_nodes_cap;
    q->wide_ws = bu_hip_malloc(ctx, bu::tsvq_wide_workspace_bytes(q->wide_blocks_cap));
    q->wide_nodes = (bu::tsvq_wide_node*)bu_hip_malloc(ctx, (size_t)q->wide_nodes_cap * sizeof(bu::tsvq_wide_node));
    q->wide_ctrl_raw = bu_hip_malloc(ctx, (size_t)q->wide_nodes_cap * sizeof(bu::tsvq_wide_ctrl));
    q->wide_ctrl = static_cast<bu::tsvq_wide_ctrl*>(q->wide_ctrl_raw);
    q->wide_packed = bu_hip_malloc(ctx, (size_t)n * member_bytes);
    return q->wide_ws && q->wide_nodes && q->wide_ctrl && q->wide_packed;
}

// The many-workgroup record of node `s`: result slot out_index, its 256-member blocks from first_block on (which moves past them). Weight and origin: zero but for splits.
static bu::tsvq_wide_node tsvq_wide_node_of(const bu_tsvq_node& s, uint32_t out_index, uint32_t& first_block, bool for_split) {
    bu::tsvq_wide_node w; std::memset(&w, 0, sizeof(w));
    w.buf = s.buf; w.start = s.start; w.count = s.count; w.out_index = out_index; w.first_block = first_block; w.n_blocks = (s.count + 255) / 256;
    if (for_split) { w.weight = s.weight; std::memcpy(w.origin, s.origin, sizeof(w.origin)); }
    first_block += w.n_blocks;
    return w;
}

// One staged round trip: in_bytes of records from the page-locked buffer to d_in, `launch` (0 = failed, error text set) timed as `region`, a wait for it where drain_first (the span roots have one, the splits' redo rounds never had), out_bytes of q->outs back into that buffer.
template <class Launch> static int tsvq_staged_round(bu_hip_context* ctx, bu_tsvq* q, const char* region, bool drain_first, void* d_in, size_t in_bytes, size_t out_bytes, Launch launch) {
    BU_TRY(ctx, hipMemcpyAsync(d_in, q->pinned, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    {
        prof_scope ps(ctx, region);
        if (!launch()) return 0;
    }
    if (drain_first) BU_TRY(ctx, stream_wait(ctx, ctx->stream));   // the node records were read from the pinned buffer the results come back to
    BU_TRY(ctx, hipMemcpyAsync(q->pinned, q->outs.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}

extern "C" {
void bu_hip_tsvq_destroy(bu_hip_context* ctx, bu_tsvq* q) {
    if (!ctx || !q) return;
    device_guard g(ctx->device);
    (void)stream_wait(ctx, ctx->stream);
    for (void* p : {q->rows, (void*)q->w64, (void*)q->perm[0], (void*)q->side, q->nodes.p, q->outs.p, q->deep_nodes.p, q->xchg, q->wide_ws, q->wide_packed, (void*)q->wide_nodes, q->wide_ctrl_raw}) if (p) bu_hip_free(ctx, p);
    q->nodes.p = nullptr; q->outs.p = nullptr; q->deep_nodes.p = nullptr;
    if (q->pinned) {  // hand the pinned staging buffer back to the context (keep the larger one)
        if (q->pinned_cap > ctx->tsvq_pinned_cap) { if (ctx->tsvq_pinned) (void)hipHostFree(ctx->tsvq_pinned); ctx->tsvq_pinned = q->pinned; ctx->tsvq_pinned_cap = q->pinned_cap; }
        else (void)hipHostFree(q->pinned);
    }
    delete q;
}

static bu_tsvq* tsvq_create_common(bu_hip_context* ctx, uint32_t dim, bool packed, const void* h_rows, const uint64_t* h_weights, uint32_t n, bu_tsvq_root* out_root,
                                   bool source_on_device = false, const uint64_t* d_endpoint_keys = nullptr, const uint32_t* d_endpoint_goffs = nullptr) {
    if (!ctx || !n || !out_root || (dim != 6 && dim != 16) || (packed && dim != 16)) { if (ctx) set_error(ctx, "tsvq_create: bad arguments"); return nullptr; }
    device_guard g(ctx->device);
    bu_tsvq* q = new (std::nothrow) bu_tsvq();
    if (!q) return nullptr;
    q->dim = dim; q->n = n; q->packed = packed;
    const bu_hip_tuning& tune = ctx->tuning;
    q->force_chained = tune.tsvq_chained_only != 0;
    q->zero_copy = tune.tsvq_zero_copy != 0;
    q->dbg_rounds = (tune.debug & 1) != 0; q->dbg_serial = (tune.debug & 2) != 0; q->dbg_stats = (tune.debug & 4) != 0;
    q->windows = (int)tune.tsvq_windows; q->dense_min = tune.tsvq_dense_min; q->poll = (int)tune.tsvq_poll;
    const size_t row_bytes = packed ? 4 : (size_t)dim * 4;
    auto fail = [&](const char* what) -> bu_tsvq* { set_error(ctx, "tsvq_create: %s", what); bu_hip_tsvq_destroy(ctx, q); return nullptr; };
    if (ctx->tsvq_pinned) { q->pinned = ctx->tsvq_pinned; q->pinned_cap = ctx->tsvq_pinned_cap; ctx->tsvq_pinned = nullptr; ctx->tsvq_pinned_cap = 0; }
    // all device blocks come from (and return to) the context's pool; the node / result records are sized for the largest batch
    // a codebook of cMaxSelectorClusters can ask for, so they never grow
    const size_t rec_cap = (size_t)16384 * std::max(sizeof(bu_tsvq_node), sizeof(bu_tsvq_split));
    q->rows = bu_hip_malloc(ctx, (size_t)n * row_bytes); q->w64 = (uint64_t*)bu_hip_malloc(ctx, (size_t)n * 8);
    q->perm[0] = (uint32_t*)bu_hip_malloc(ctx, (size_t)n * 4 * bu::TSVQ_BUFS); q->perm[1] = q->perm[0] ? q->perm[0] + n : nullptr;
    q->side = (uint8_t*)bu_hip_malloc(ctx, n);
    q->nodes.p = bu_hip_malloc(ctx, rec_cap); q->outs.p = bu_hip_malloc(ctx, rec_cap);
    if (!q->rows || !q->w64 || !q->perm[0] || !q->perm[1] || !q->side || !q->nodes.p || !q->outs.p) return fail("allocation");
    q->nodes.cap = q->outs.cap = rec_cap;
    // the endpoint tree's large nodes through the many-workgroup path for 6-float rows (tsvq_wide6_kernels.hip): tsvq_wide6_min, default 8,192
    // (6,144 / 10,000 / 14,000 side by side on one box: 1.68 / 1.69 / 1.69 ms for the endpoint tree's splits, 2.15 without the path); 0 = off (tests compare both)
    if (!packed && dim == 6 && !q->force_chained && !tsvq_alloc_wide(ctx, q, tune.tsvq_wide6_min, 32, 0)) return fail("allocation");   // (32: the list-order copies of the per-member addends, 6 n floats + n doubles)
    // packed rows: tsvq_wide_min, default 8,192 (16,384 until round 3: the one-workgroup launches of the smaller nodes are the longer of the two concurrent streams);
    // tsvq_wide_cov_min, default 98,304 (side by side on one box with the register-composed stretches kernel: 131,072 / 98,304 / 65,536 / 49,152 -> 5.10 / 4.98 / 5.04 / 5.04 ms
    // of many-workgroup rounds per 4096^2 step)
    if (packed && !q->force_chained && !tsvq_alloc_wide(ctx, q, tune.tsvq_wide_min, 8, tune.tsvq_wide_cov_min)) return fail("allocation");
    if (d_endpoint_keys) {   // the rows are made on the device from the de-duplication's keys (bu_hip_k_unique_endpoint_vectors)
        if (bu::launch_endpoint_rows(ctx->stream, d_endpoint_keys, d_endpoint_goffs, n, static_cast<float*>(q->rows), q->w64) != hipSuccess) return fail("endpoint rows");
    } else if (source_on_device) {  // stream-ordered device copies: the vectors were produced on this context's stream
        if (hipMemcpyAsync(q->rows, h_rows, (size_t)n * row_bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(q->w64, h_weights, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
            return fail("device copy");
    } else if (stream_wait(ctx, ctx->stream) != hipSuccess || hipMemcpy(q->rows, h_rows, (size_t)n * row_bytes, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(q->w64, h_weights, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail("upload");  // blocking copies (the sources are pageable, see bu_tsvq::pinned); the root kernel below needs both anyway
    // the page-locked buffer here: [0] the root's node record (many-workgroup variant), [256] the root record the kernels produce, [768] the completion word
    constexpr size_t ROOT_AT = 256, FLAG_AT = 768;
    static_assert(sizeof(bu::tsvq_wide_node) <= ROOT_AT && ROOT_AT + sizeof(bu_tsvq_root) <= FLAG_AT, "layout of the root's page-locked records");
    if (q->reserve_pinned(1024) != hipSuccess) return fail("pinned allocation");
    // Zero-copy (as the rounds, tsvq_split_impl): the kernels read the node record from and write the root record into the page-locked buffer and a last one-thread kernel
    // stores a word there that this thread looks at -- no copy commands, no hipStreamSynchronize between the root and the first round.
    char* d_pinned = nullptr;
    if (q->zero_copy && hipHostGetDevicePointer(reinterpret_cast<void**>(&d_pinned), q->pinned, 0) != hipSuccess) { (void)hipGetLastError(); d_pinned = nullptr; }
    bu::tsvq_root_out* d_root = d_pinned ? reinterpret_cast<bu::tsvq_root_out*>(d_pinned + ROOT_AT) : static_cast<bu::tsvq_root_out*>(q->outs.p);
    const bu_tsvq_root* h_root = reinterpret_cast<const bu_tsvq_root*>(static_cast<const char*>(q->pinned) + (d_pinned ? ROOT_AT : 0));
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(static_cast<char*>(q->pinned) + FLAG_AT);
    // many-workgroup variant first where it applies, then the exact (integer-reduced) one-workgroup variant; a record flagged
    // pad == 1 left the exact range -> next variant, the chained one last
    for (int attempt = q->wide_min ? -1 : 0; attempt < 2; attempt++) {
        const bool exact = packed && attempt == 0 && !q->force_chained;
        if (d_pinned) { *flag = 0; }
        if (attempt < 0) {
            bu_tsvq_node whole{}; whole.count = n; uint32_t first = 0;   // the training set in its first order: buffer 0 from 0
            const bu::tsvq_wide_node wn = tsvq_wide_node_of(whole, 0, first, false);
            std::memcpy(q->pinned, &wn, sizeof(wn));
            if (d_pinned) {
                __atomic_thread_fence(__ATOMIC_SEQ_CST);
                if (bu::launch_tsvq_wide_prologue(ctx->stream, reinterpret_cast<const bu::tsvq_wide_node*>(d_pinned), q->wide_nodes, q->wide_ctrl, 1) != hipSuccess) return fail("root upload");
            } else if (hipMemcpyAsync(q->wide_nodes, q->pinned, sizeof(wn), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("root upload");
            prof_scope ps(ctx, packed ? "tsvq_root_packed16" : "tsvq_root_float6");
            if (!packed) {
                if (bu::launch_tsvq_wide6_root(ctx->stream, static_cast<const float*>(q->rows), q->w64, n, q->perm[0], q->side, q->wide_nodes, q->wide_ctrl, q->wide_ws, wn.n_blocks,
                                               d_root, static_cast<float*>(q->wide_packed),
                                               reinterpret_cast<double*>(static_cast<char*>(q->wide_packed) + (size_t)n * 24), d_pinned != nullptr) != hipSuccess) return fail("wide root launch");
            } else
            if (bu::launch_tsvq_wide_root(ctx->stream, static_cast<const uint32_t*>(q->rows), q->w64, n, q->perm[0], q->wide_nodes, q->wide_ctrl, q->wide_ws, wn.n_blocks,
                                          d_root, q->windows, d_pinned != nullptr) != hipSuccess) return fail("wide root launch");
        } else {
            if (d_pinned) __atomic_thread_fence(__ATOMIC_SEQ_CST);
            prof_scope ps(ctx, packed ? "tsvq_root_packed16" : "tsvq_root_float6");
            if (bu::launch_tsvq_root(ctx->stream, (int)dim, packed, exact, q->rows, q->w64, n, q->perm[0], d_root) != hipSuccess) return fail("root launch");
        }
        if (d_pinned) {
            const uint32_t seq = next_seq(q->round_seq);
            if (bu::launch_tsvq_signal(ctx->stream, reinterpret_cast<uint32_t*>(d_pinned + FLAG_AT), seq) != hipSuccess || !wait_flag(ctx, q->poll, flag, seq, "tsvq_create")) return fail("root wait");
        } else if (hipMemcpyAsync(q->pinned, q->outs.p, sizeof(bu_tsvq_root), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || stream_wait(ctx, ctx->stream) != hipSuccess)
            return fail("root download");
        if ((attempt >= 0 && !exact) || h_root->pad == 0) break;
    }
    std::memcpy(out_root, h_root, sizeof(bu_tsvq_root));
    return q;
}

bu_tsvq* bu_hip_tsvq_create(bu_hip_context* ctx, uint32_t dim, const float* h_rows, const uint64_t* h_weights, uint32_t n, bu_tsvq_root* out_root) {
    return tsvq_create_common(ctx, dim, false, h_rows, h_weights, n, out_root);
}

bu_tsvq* bu_hip_tsvq_create_packed16(bu_hip_context* ctx, const uint32_t* h_keys, const uint64_t* h_weights, uint32_t n, bu_tsvq_root* out_root) {
    return tsvq_create_common(ctx, 16, true, h_keys, h_weights, n, out_root);
}

bu_tsvq* bu_hip_tsvq_create_packed16_device(bu_hip_context* ctx, const uint32_t* d_keys, const uint64_t* d_weights, uint32_t n, bu_tsvq_root* out_root) {
    return tsvq_create_common(ctx, 16, true, d_keys, d_weights, n, out_root, true);
}

bu_tsvq* bu_hip_tsvq_create_endpoint_device(bu_hip_context* ctx, const uint64_t* d_unique_keys, const uint32_t* d_group_offsets, uint32_t n, bu_tsvq_root* out_root) {
    if (ctx && (!d_unique_keys || !d_group_offsets)) { set_error(ctx, "tsvq_create_endpoint_device: null pointer"); return nullptr; }
    return tsvq_create_common(ctx, 6, false, nullptr, nullptr, n, out_root, true, d_unique_keys, d_group_offsets);
}

// One round of splits. levels > 0 (deep round, zero-copy rounds only): the one-workgroup nodes' children, grandchildren, ... are split in the same round trip --
// every generation's node records are made on the device from the results of the one before (k_tsvq_children), so `levels` more launches follow the batch's own
// without the host. h_deep: generation g (1..levels) of batch node i, path p (the sides taken, first step in the top bit) at h_deep[n_nodes * (2^g - 2) + i * 2^g + p];
// ok == 3 = not attempted (the parent's split failed or went through the many-workgroup passes, one member, variance below the floor in h_nodes[i].pad).
static int tsvq_split_impl(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_split* h_out, uint32_t levels, bu_tsvq_split* h_deep) {
    if (!ctx || !q) return 0;
    if (!n_nodes) return 1;
    // as bu_hip_tsvq_roots: a record that is no span of the member buffers is refused here, before anything is launched (the kernels index with it as it stands)
    for (uint32_t i = 0; i < n_nodes; i++)
        if (h_nodes[i].buf >= bu::TSVQ_BUFS || !h_nodes[i].count || (uint64_t)h_nodes[i].start + h_nodes[i].count > q->n) { set_error(ctx, "tsvq_split: span outside the training set"); return 0; }
    if (levels > bu::TSVQ_MAX_DEEP_LEVELS) levels = bu::TSVQ_MAX_DEEP_LEVELS;   // tsvq_bufs.h: a write must not reach a list that may still become a leaf
    const uint32_t h_deep_levels = h_deep ? levels : 0;   // what the caller's array is laid out for (the round may attempt fewer)
    device_guard g(ctx->device);
    const bool round_stats = q->dbg_rounds;   // development aid: one line per round on stderr
    const auto round_t0 = std::chrono::steady_clock::now();
    if ((size_t)n_nodes * sizeof(bu_tsvq_node) > q->nodes.cap || (size_t)n_nodes * sizeof(bu_tsvq_split) > q->outs.cap) { set_error(ctx, "tsvq_split: batch of %u nodes exceeds the record buffers", n_nodes); return 0; }
    // Large nodes go through the many-workgroup path, the rest one workgroup each; both write one result array
    // (narrow records first, in batch order, then the wide ones).
    std::vector<uint32_t> order; order.reserve(n_nodes);
    uint32_t n_wide = 0, wide_blocks = 0, wide_max_count = 0;
    uint64_t wide_max_weight = 0;   // chain addends are value (0..3) x weight: 3 x a node's weight bounds every side chain's total
    if (q->wide_min) {
        std::vector<uint32_t> wide;
        for (uint32_t i = 0; i < n_nodes; i++) {
            const uint32_t nb = (h_nodes[i].count + 255) / 256;
            if (h_nodes[i].count >= q->wide_min && (q->packed || h_nodes[i].weight < (1ull << 52)) && wide.size() < q->wide_nodes_cap && wide_blocks + nb <= q->wide_blocks_cap) { wide.push_back(i); wide_blocks += nb; wide_max_count = std::max(wide_max_count, h_nodes[i].count); wide_max_weight = std::max<uint64_t>(wide_max_weight, h_nodes[i].weight); }
            else order.push_back(i);
        }
        n_wide = (uint32_t)wide.size();
        order.insert(order.end(), wide.begin(), wide.end());
    } else for (uint32_t i = 0; i < n_nodes; i++) order.push_back(i);
    const uint32_t n_narrow = n_nodes - n_wide;
    const size_t in_bytes = (size_t)n_narrow * sizeof(bu_tsvq_node), wide_bytes = (size_t)n_wide * sizeof(bu::tsvq_wide_node), out_bytes = (size_t)n_nodes * sizeof(bu_tsvq_split);
    const size_t wide_at = (in_bytes + 63) & ~(size_t)63;
    const bool zero_copy = q->zero_copy;
    // staged: the result records come back over the node records; zero-copy: the kernels write them while others still read their nodes, so they get their own place
    if (!zero_copy || !n_narrow || q->dbg_serial || !h_deep) levels = 0;
    while (levels && (size_t)n_narrow * ((2u << levels) - 2u) * sizeof(bu_tsvq_split) > ((size_t)64 << 20)) levels--;   // (never in practice: 64 MiB of records)
    const size_t deep_recs = (size_t)n_narrow * ((2u << levels) - 2u);   // 2 + 4 + ... + 2^levels per one-workgroup node
    const size_t out_at = zero_copy ? ((wide_at + wide_bytes + 63) & ~(size_t)63) : 0, deep_at = out_at + out_bytes,
                 flag_at = (deep_at + deep_recs * sizeof(bu_tsvq_split) + 63) & ~(size_t)63;
    BU_TRY(ctx, q->reserve_pinned(std::max(wide_at + wide_bytes, flag_at + 128)));   // the round's flag
    if (deep_recs * sizeof(bu_tsvq_node) > q->deep_nodes.cap) {
        if (q->deep_nodes.p) { BU_TRY(ctx, stream_wait(ctx, ctx->stream)); bu_hip_free(ctx, q->deep_nodes.p); q->deep_nodes.p = nullptr; q->deep_nodes.cap = 0; }
        const size_t want = deep_recs * sizeof(bu_tsvq_node) * 2;
        q->deep_nodes.p = bu_hip_malloc(ctx, want);
        if (!q->deep_nodes.p) { set_error(ctx, "tsvq_split: allocation of %zu bytes of node records failed", want); return 0; }
        q->deep_nodes.cap = want;
    }
    char* d_pinned = nullptr;   // the page-locked buffer as the device addresses it
    if (zero_copy) BU_TRY(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&d_pinned), q->pinned, 0));
    volatile uint32_t* round_flag = reinterpret_cast<volatile uint32_t*>(static_cast<char*>(q->pinned) + flag_at);
    const bu::tsvq_node_in* d_nodes_in = zero_copy ? reinterpret_cast<const bu::tsvq_node_in*>(d_pinned) : static_cast<const bu::tsvq_node_in*>(q->nodes.p);
    bu::tsvq_split_out* d_outs = zero_copy ? reinterpret_cast<bu::tsvq_split_out*>(d_pinned + out_at) : static_cast<bu::tsvq_split_out*>(q->outs.p);
    {
        bu_tsvq_node* pn = static_cast<bu_tsvq_node*>(q->pinned);
        for (uint32_t i = 0; i < n_narrow; i++) pn[i] = h_nodes[order[i]];
        bu::tsvq_wide_node* pw = reinterpret_cast<bu::tsvq_wide_node*>(static_cast<char*>(q->pinned) + wide_at);
        uint32_t first = 0;
        for (uint32_t i = 0; i < n_wide; i++) pw[i] = tsvq_wide_node_of(h_nodes[order[n_narrow + i]], n_narrow + i, first, true);
    }
    if (zero_copy) { *round_flag = 0; __atomic_thread_fence(__ATOMIC_SEQ_CST); }
    if (n_narrow && !zero_copy) BU_TRY(ctx, hipMemcpyAsync(q->nodes.p, q->pinned, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    // the wide nodes' records + their cleared state: one kernel that reads the page-locked records, where the device can address them (otherwise a copy here and a fill in the launcher)
    const bool wide_prologue = n_wide && zero_copy;
    if (wide_prologue) BU_TRY(ctx, bu::launch_tsvq_wide_prologue(ctx->stream, reinterpret_cast<const bu::tsvq_wide_node*>(d_pinned + wide_at), q->wide_nodes, q->wide_ctrl, n_wide));
    else if (n_wide) BU_TRY(ctx, hipMemcpyAsync(q->wide_nodes, static_cast<char*>(q->pinned) + wide_at, wide_bytes, hipMemcpyHostToDevice, ctx->stream));
    const bool exact = q->packed && !q->force_chained;
    // The two kinds of node of a round do not touch each other's data: when both are present the one-workgroup kernel runs on the side
    // stream, under the many small launches of the wide path. (Not while kernels are being timed one by one.)
    bool narrow_on_side = n_wide && n_narrow && ctx->profiling != 1 && !q->dbg_serial;   // (not while the rounds' kernels are being timed one region after the other)
    if (narrow_on_side && !ensure_side_stream(ctx)) narrow_on_side = false;
    // deep round: generation g's records from generation g - 1's results, then its splits, on the stream the batch's own one-workgroup launch went to
    auto deep_generations = [&](hipStream_t st) -> bool {
        const bu::tsvq_node_in* parents = d_nodes_in;
        const bu::tsvq_split_out* parent_outs = d_outs;
        bu::tsvq_node_in* children = static_cast<bu::tsvq_node_in*>(q->deep_nodes.p);
        bu::tsvq_split_out* child_outs = reinterpret_cast<bu::tsvq_split_out*>(d_pinned + deep_at);
        uint32_t n_parents = n_narrow;
        for (uint32_t gen = 1; gen <= levels; gen++) {
            if (bu::launch_tsvq_children(st, parents, parent_outs, n_parents, children, child_outs) != hipSuccess ||
                q->launch_split(st, exact, children, 2 * n_parents, child_outs) != hipSuccess) {
                set_error(ctx, "tsvq_split: deep generation %u: %s", gen, hipGetErrorString(hipGetLastError()));
                return false;
            }
            parents = children; parent_outs = child_outs;
            children += 2 * (size_t)n_parents; child_outs += 2 * (size_t)n_parents;
            n_parents *= 2;
        }
        return true;
    };
    // From the fork on, every early return must wait for the side stream first: the caller's guard destroys q (its buffers go back to the
    // pool without a synchronisation) while the one-workgroup kernel may still be running on them.
    struct side_joiner { hipStream_t s; bool armed; ~side_joiner() { if (armed) (void)hipStreamSynchronize(s); } } side_join_guard{ctx->side_stream, false};
    if (narrow_on_side) {
        side_join_guard.s = ctx->side_stream; side_join_guard.armed = true;
        BU_TRY(ctx, hipEventRecord(ctx->side_fork, ctx->stream));
        BU_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
        BU_TRY(ctx, q->launch_split(ctx->side_stream, exact, d_nodes_in, n_narrow, d_outs));
        if (levels && !deep_generations(ctx->side_stream)) return 0;
        BU_TRY(ctx, hipEventRecord(ctx->side_join, ctx->side_stream));
    }
    if (n_wide) {
        prof_scope ps(ctx, q->packed ? "tsvq_split_packed16_wide" : "tsvq_split_float6_wide");
        if (!q->packed)
            BU_TRY(ctx, bu::launch_tsvq_wide6_split(ctx->stream, static_cast<const float*>(q->rows), q->w64, q->n, q->perm[0], q->perm[1], q->side, q->wide_nodes, n_wide, q->wide_ctrl, q->wide_ws,
                                                    wide_blocks, d_outs, static_cast<float*>(q->wide_packed), reinterpret_cast<double*>(static_cast<char*>(q->wide_packed) + (size_t)q->n * 24), wide_prologue));
        else
        BU_TRY(ctx, bu::launch_tsvq_wide_split(ctx->stream, static_cast<const uint32_t*>(q->rows), q->w64, q->perm[0], q->perm[1], q->side, q->wide_packed, q->wide_nodes, n_wide, q->wide_ctrl,
                                               q->wide_ws, wide_blocks, d_outs, wide_max_count < q->wide_cov_min,
                                               wide_max_weight * 3ull < (1ull << 24), q->windows, wide_prologue));
    }
    if (n_wide && q->dbg_stats && q->packed) {   // development aid: how the last pass's walks went, per wide node
        std::vector<bu::tsvq_wide_ctrl> hc(n_wide);
        if (d2h_pageable(ctx, hc.data(), q->wide_ctrl, hc.size() * sizeof(bu::tsvq_wide_ctrl)) == hipSuccess && stream_wait(ctx, ctx->stream) == hipSuccess)
            for (uint32_t i = 0; i < n_wide; i++) {
                uint32_t ms = 0, mr = 0, ts = 0, tr = 0, ex = 0;
                for (int c = 0; c < 32; c++) { ms = std::max<uint32_t>(ms, hc[i].stat_scans[c]); mr = std::max<uint32_t>(mr, hc[i].stat_raw[c]); ts += hc[i].stat_scans[c]; tr += hc[i].stat_raw[c]; ex += hc[i].exact[c]; }
                std::fprintf(stderr, "[tsvq stats] wide node %u: count %u blocks %u iter %d | last pass, 32 side chains: scans max %u avg %.1f, raw blocks max %u avg %.1f, exact chains %u\n",
                             i, h_nodes[order[n_narrow + i]].count, (h_nodes[order[n_narrow + i]].count + 255) / 256, hc[i].iter, ms, ts / 32.0, mr, tr / 32.0, ex);
                uint32_t cms = 0, cmr = 0, cts = 0, ctr = 0, diag_r = 0; int x = 0, y = 0;
                for (int c = 0; c < 136; c++) {
                    cms = std::max<uint32_t>(cms, hc[i].stat_cov_scans[c]); cmr = std::max<uint32_t>(cmr, hc[i].stat_cov_raw[c]); cts += hc[i].stat_cov_scans[c]; ctr += hc[i].stat_cov_raw[c];
                    if (x == y) diag_r += hc[i].stat_cov_raw[c];
                    if (++y == 16) { x++; y = x; }
                }
                if (cts) std::fprintf(stderr, "[tsvq stats]      covariance pass, 136 chains: scans max %u avg %.1f, raw blocks max %u avg %.1f (diagonal avg %.1f)\n", cms, cts / 136.0, cmr, ctr / 136.0, diag_r / 16.0);
            }
    }
    if (narrow_on_side) { BU_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_join, 0)); side_join_guard.armed = false; }
    else if (n_narrow) {
        prof_scope ps(ctx, q->packed ? "tsvq_split_packed16" : "tsvq_split_float6");
        BU_TRY(ctx, q->launch_split(ctx->stream, exact, d_nodes_in, n_narrow, d_outs));
        if (levels && !deep_generations(ctx->stream)) return 0;
    }
    if (zero_copy) {
        const uint32_t seq = next_seq(q->round_seq);
        BU_TRY(ctx, bu::launch_tsvq_signal(ctx->stream, reinterpret_cast<uint32_t*>(d_pinned + flag_at), seq));
        if (!wait_flag(ctx, q->poll, round_flag, seq, "tsvq_split")) return 0;
    } else {
        BU_TRY(ctx, hipMemcpyAsync(q->pinned, q->outs.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    }
    if (round_stats) {
        uint32_t mx = 0; uint64_t tot = 0;
        for (uint32_t i = 0; i < n_nodes; i++) { mx = std::max(mx, h_nodes[i].count); tot += h_nodes[i].count; }
        std::fprintf(stderr, "[tsvq round] dim %u: %u nodes (%u wide), largest %u, members %llu: %.0f us\n", q->dim, n_nodes, n_wide, mx, (unsigned long long)tot,
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - round_t0).count());
    }
    {
        const bu_tsvq_split* po = reinterpret_cast<const bu_tsvq_split*>(static_cast<const char*>(q->pinned) + out_at);
        for (uint32_t i = 0; i < n_nodes; i++) h_out[order[i]] = po[i];
    }
    if (h_deep) {   // generation g of batch node i, path p: h_deep[n_nodes * (2^g - 2) + i * 2^g + p]; here generation g of one-workgroup node j sits at pd[n_narrow * (2^g - 2) + j * 2^g + p]
        const bu_tsvq_split* pd = reinterpret_cast<const bu_tsvq_split*>(static_cast<const char*>(q->pinned) + deep_at);
        for (uint32_t gen = 1; gen <= h_deep_levels; gen++) {
            bu_tsvq_split* dst = h_deep + (size_t)n_nodes * ((1u << gen) - 2u);
            const uint32_t w = 1u << gen;
            if (gen > levels) { for (size_t k = 0; k < (size_t)n_nodes * w; k++) dst[k].ok = 3; continue; }
            const bu_tsvq_split* src = pd + (size_t)n_narrow * (w - 2u);
            for (uint32_t j = 0; j < n_nodes; j++) {
                bu_tsvq_split* d = dst + (size_t)order[j] * w;
                if (j >= n_narrow) { for (uint32_t p2 = 0; p2 < w; p2++) d[p2].ok = 3; continue; }
                for (uint32_t p2 = 0; p2 < w; p2++) {
                    const bu_tsvq_split& r = src[(size_t)j * w + p2];
                    if (r.ok == 1 || r.ok == 0) d[p2] = r; else d[p2].ok = 3;   // (ok == 2, data outside the exact kernel's range: left to a later round, which has the redo path)
                }
            }
        }
    }
    if (exact || n_wide) { // nodes whose data left the exact range, or that a wide path handed back (ok == 2), go through the one-workgroup kernel: packed wide ones through its exact variant first
        for (int attempt = exact ? 0 : 1; attempt < 2; attempt++) {
            std::vector<uint32_t> redo;
            for (uint32_t i = 0; i < n_nodes; i++) if (h_out[i].ok == 2) redo.push_back(i);
            if (redo.empty()) break;
            bu_tsvq_node* pn = static_cast<bu_tsvq_node*>(q->pinned);
            for (size_t j = 0; j < redo.size(); j++) pn[j] = h_nodes[redo[j]];
            if (!tsvq_staged_round(ctx, q, q->packed ? "tsvq_split_packed16" : "tsvq_split_float6", false, q->nodes.p, redo.size() * sizeof(bu_tsvq_node), redo.size() * sizeof(bu_tsvq_split), [&]() -> int {
                    BU_TRY(ctx, q->launch_split(ctx->stream, exact && attempt == 0 && n_wide != 0, static_cast<const bu::tsvq_node_in*>(q->nodes.p), (uint32_t)redo.size(), static_cast<bu::tsvq_split_out*>(q->outs.p)));
                    return 1;
                })) return 0;
            const bu_tsvq_split* po = static_cast<const bu_tsvq_split*>(q->pinned);
            for (size_t j = 0; j < redo.size(); j++) h_out[redo[j]] = po[j];
        }
    }
    return 1;
}

int bu_hip_tsvq_split(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_split* h_out) {
    return tsvq_split_impl(ctx, q, h_nodes, n_nodes, h_out, 0, nullptr);
}

int bu_hip_tsvq_split_deep(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_split* h_out, uint32_t levels, bu_tsvq_split* h_deep) {
    if (levels && !h_deep) { if (ctx) set_error(ctx, "tsvq_split_deep: no array for the deeper generations"); return 0; }
    if (levels > bu::TSVQ_MAX_DEEP_LEVELS) { if (ctx) set_error(ctx, "tsvq_split_deep: %u levels (at most BU_TSVQ_BUFFERS - 2)", levels); return 0; }
    return tsvq_split_impl(ctx, q, h_nodes, n_nodes, h_out, levels, h_deep);
}

// prepare_root (enc.h:1708-1735) of member spans: what a tree_vector_quant whose training set is that span, in list order, starts from --
// the roots of the T independent trees of generate_hierarchical_codebook_threaded_internal (enc.h:2137-2152).
int bu_hip_tsvq_roots(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_root* h_out) {
    if (!ctx || !q || (n_nodes && (!h_nodes || !h_out))) return 0;
    if (!n_nodes) return 1;
    device_guard g(ctx->device);
    if ((size_t)n_nodes * sizeof(bu_tsvq_node) > q->nodes.cap) { set_error(ctx, "tsvq_roots: %u spans exceed the record buffer", n_nodes); return 0; }
    for (uint32_t i = 0; i < n_nodes; i++)
        if (h_nodes[i].buf >= bu::TSVQ_BUFS || !h_nodes[i].count || (uint64_t)h_nodes[i].start + h_nodes[i].count > q->n) { set_error(ctx, "tsvq_roots: span outside the training set"); return 0; }
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));   // the pinned staging buffer may still feed an earlier copy
    BU_TRY(ctx, q->reserve_pinned((size_t)n_nodes * std::max(std::max(sizeof(bu_tsvq_node), sizeof(bu_tsvq_root)), sizeof(bu::tsvq_wide_node))));
    std::vector<uint32_t> todo;
    // large spans of packed rows: the many-workgroup root pass (one batch); a record flagged pad == 1 left its exact range -> the one-workgroup kernels below
    if (q->wide_min && q->packed) {
        std::vector<uint32_t> wide;
        uint32_t blocks = 0;
        for (uint32_t i = 0; i < n_nodes; i++) {
            const uint32_t nb = (h_nodes[i].count + 255) / 256;
            if (h_nodes[i].count >= q->wide_min && wide.size() < q->wide_nodes_cap && blocks + nb <= q->wide_blocks_cap) { wide.push_back(i); blocks += nb; }
            else todo.push_back(i);
        }
        if (!wide.empty()) {
            bu::tsvq_wide_node* pw = static_cast<bu::tsvq_wide_node*>(q->pinned);
            uint32_t first = 0;
            for (size_t j = 0; j < wide.size(); j++) pw[j] = tsvq_wide_node_of(h_nodes[wide[j]], (uint32_t)j, first, false);
            if (!tsvq_staged_round(ctx, q, "tsvq_root_packed16", true, q->wide_nodes, wide.size() * sizeof(bu::tsvq_wide_node), wide.size() * sizeof(bu_tsvq_root), [&]() -> int {
                    BU_TRY(ctx, bu::launch_tsvq_wide_span_roots(ctx->stream, static_cast<const uint32_t*>(q->rows), q->w64, q->perm[0], q->perm[1], q->wide_packed, q->wide_nodes,
                                                                (uint32_t)wide.size(), q->wide_ctrl, q->wide_ws, blocks, static_cast<bu::tsvq_root_out*>(q->outs.p), q->windows));
                    return 1;
                })) return 0;
            const bu_tsvq_root* po = static_cast<const bu_tsvq_root*>(q->pinned);
            for (size_t j = 0; j < wide.size(); j++) {
                if (po[j].pad) todo.push_back(wide[j]); else h_out[wide[j]] = po[j];
            }
            std::sort(todo.begin(), todo.end());
        }
    } else {
        todo.resize(n_nodes);
        for (uint32_t i = 0; i < n_nodes; i++) todo[i] = i;
    }
    // the exact (integer-reduced) variant first where it applies; a record flagged pad == 1 left the exact range -> the chained one
    for (int attempt = (q->packed && !q->force_chained) ? 0 : 1; attempt < 2 && !todo.empty(); attempt++) {
        bu_tsvq_node* pn = static_cast<bu_tsvq_node*>(q->pinned);
        for (size_t j = 0; j < todo.size(); j++) pn[j] = h_nodes[todo[j]];
        if (!tsvq_staged_round(ctx, q, q->packed ? "tsvq_root_packed16" : "tsvq_root_float6", true, q->nodes.p, todo.size() * sizeof(bu_tsvq_node), todo.size() * sizeof(bu_tsvq_root), [&]() -> int {
                BU_TRY(ctx, bu::launch_tsvq_span_roots(ctx->stream, (int)q->dim, q->packed, attempt == 0, q->rows, q->w64, q->perm[0], q->perm[1],
                                                       static_cast<const bu::tsvq_node_in*>(q->nodes.p), (uint32_t)todo.size(), static_cast<bu::tsvq_root_out*>(q->outs.p)));
                return 1;
            })) return 0;
        const bu_tsvq_root* po = static_cast<const bu_tsvq_root*>(q->pinned);
        std::vector<uint32_t> redo;
        for (size_t j = 0; j < todo.size(); j++) {
            if (attempt == 0 && po[j].pad) redo.push_back(todo[j]);
            else h_out[todo[j]] = po[j];
        }
        todo.swap(redo);
    }
    return 1;
}

static_assert(sizeof(bu_tsvq_span) == sizeof(bu::bk_span), "layout");
int bu_hip_tsvq_scatter_spans(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_span* h_spans, uint32_t n_spans, uint32_t* d_out) {
    if (!ctx || !q || (n_spans && (!h_spans || !d_out))) return 0;
    if (!n_spans) return 1;
    device_guard g(ctx->device);
    const size_t bytes = (size_t)n_spans * sizeof(bu_tsvq_span);
    if (bytes > q->nodes.cap) { set_error(ctx, "tsvq_scatter_spans: %u spans exceed the record buffer", n_spans); return 0; }
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));   // the pinned staging buffer may still feed an earlier copy
    BU_TRY(ctx, q->reserve_pinned(bytes));
    std::memcpy(q->pinned, h_spans, bytes);
    BU_TRY(ctx, hipMemcpyAsync(q->nodes.p, q->pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    BU_TRY(ctx, bu::launch_scatter_spans(ctx->stream, q->perm[0], q->perm[1], static_cast<const bu::bk_span*>(q->nodes.p), n_spans, d_out));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));   // q may be destroyed (and the pinned buffer recycled) right after
    return 1;
}

int bu_hip_tsvq_finish_spans(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_span* h_spans, uint32_t n_spans, uint32_t* d_leaf_of, uint32_t* d_parent_of, const uint32_t* d_group_offsets,
                             uint32_t* d_first_pos, uint32_t* d_sizes) {
    if (!ctx || !q || (n_spans && (!h_spans || !d_leaf_of)) || (d_group_offsets && (!d_first_pos || !d_sizes))) return 0;
    if (!n_spans) return 1;
    device_guard g(ctx->device);
    const size_t bytes = (size_t)n_spans * sizeof(bu_tsvq_span);
    if (bytes > q->nodes.cap) { set_error(ctx, "tsvq_finish_spans: %u spans exceed the record buffer", n_spans); return 0; }
    BU_TRY(ctx, h2d(ctx, q->nodes.p, h_spans, bytes));   // through the context's pinned ring: the caller's array may go when this returns
    BU_TRY(ctx, bu::launch_finish_spans(ctx->stream, q->perm[0], q->perm[1], static_cast<const bu::bk_span*>(q->nodes.p), n_spans, d_leaf_of, d_parent_of, d_group_offsets, d_first_pos,
                                        d_sizes));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));   // q may be destroyed right after
    return 1;
}

// staging layout: [children of node 0 | children of node 1 | ... ] u32, padded to a u64 boundary, then n_nodes result records, then the node table + flags
static int tsvq_exchange_layout(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, uint32_t n_nodes, std::vector<bu::bk_span>& table, size_t& rec_at, size_t& tab_at, size_t& total) {
    table.resize(n_nodes);
    uint64_t run = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
        if ((uint64_t)h_nodes[i].start + h_nodes[i].count > q->n) { set_error(ctx, "tsvq_exchange: node outside the training set"); return 0; }
        table[i] = bu::bk_span{h_nodes[i].buf, h_nodes[i].start, h_nodes[i].count, (uint32_t)run};
        run += h_nodes[i].count;
    }
    if (run > (uint64_t)bu::TSVQ_BUFS * q->n) { set_error(ctx, "tsvq_exchange: overlapping nodes"); return 0; }   // (every member buffer once over: the whole-tree exchange of the one-tree-per-rank build)
    rec_at = ((size_t)run * 4 + 7) & ~(size_t)7;
    tab_at = rec_at + (size_t)n_nodes * sizeof(bu_tsvq_split);
    total = tab_at + (size_t)n_nodes * sizeof(bu::bk_span) + ((size_t)n_nodes + 7 & ~(size_t)7);
    if (total > q->xchg_cap) {
        if (q->xchg) bu_hip_free(ctx, q->xchg);
        q->xchg_cap = total + total / 4 + 4096;
        q->xchg = bu_hip_malloc(ctx, q->xchg_cap);
        if (!q->xchg) { q->xchg_cap = 0; set_error(ctx, "tsvq_exchange: allocation"); return 0; }
    }
    return 1;
}

int bu_hip_tsvq_exchange_pack(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, const uint8_t* h_mine, const bu_tsvq_split* h_records, uint32_t n_nodes,
                              void** d_staging, uint64_t* n_u64) {
    if (!ctx || !q || !h_nodes || !h_mine || !h_records || !d_staging || !n_u64 || !n_nodes) return 0;
    device_guard g(ctx->device);
    std::vector<bu::bk_span> table;
    size_t rec_at, tab_at, total;
    if (!tsvq_exchange_layout(ctx, q, h_nodes, n_nodes, table, rec_at, tab_at, total)) return 0;
    char* base = static_cast<char*>(q->xchg);
    // host part of the staging buffer: records (zero where not mine), node table, flags -- one upload
    std::vector<char> host(total - rec_at, 0);
    for (uint32_t i = 0; i < n_nodes; i++) if (h_mine[i]) std::memcpy(&host[(size_t)i * sizeof(bu_tsvq_split)], &h_records[i], sizeof(bu_tsvq_split));
    std::memcpy(&host[tab_at - rec_at], table.data(), (size_t)n_nodes * sizeof(bu::bk_span));
    std::memcpy(&host[tab_at - rec_at + (size_t)n_nodes * sizeof(bu::bk_span)], h_mine, n_nodes);
    BU_TRY(ctx, h2d(ctx, base + rec_at, host.data(), host.size()));
    if (rec_at >= 8) BU_TRY(ctx, hipMemsetAsync(base + rec_at - 8, 0, 8, ctx->stream));   // the padding word of an odd child count
    BU_TRY(ctx, bu::launch_exchange_children(ctx->stream, q->perm[0], q->perm[1], reinterpret_cast<const bu::bk_span*>(base + tab_at),
                                             reinterpret_cast<const uint8_t*>(base + tab_at + (size_t)n_nodes * sizeof(bu::bk_span)), n_nodes, reinterpret_cast<uint32_t*>(base), 0));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    *d_staging = q->xchg;
    *n_u64 = tab_at / 8;
    return 1;
}

int bu_hip_tsvq_exchange_unpack(bu_hip_context* ctx, bu_tsvq* q, const bu_tsvq_node* h_nodes, const uint8_t* h_mine, bu_tsvq_split* h_records, uint32_t n_nodes) {
    if (!ctx || !q || !h_nodes || !h_mine || !h_records || !n_nodes || !q->xchg) return 0;
    device_guard g(ctx->device);
    std::vector<bu::bk_span> table;
    size_t rec_at, tab_at, total;
    if (!tsvq_exchange_layout(ctx, q, h_nodes, n_nodes, table, rec_at, tab_at, total)) return 0;
    char* base = static_cast<char*>(q->xchg);
    std::vector<uint8_t> theirs(n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) theirs[i] = h_mine[i] ? 0 : 1;
    BU_TRY(ctx, h2d(ctx, base + tab_at + (size_t)n_nodes * sizeof(bu::bk_span), theirs.data(), n_nodes));
    BU_TRY(ctx, bu::launch_exchange_children(ctx->stream, q->perm[0], q->perm[1], reinterpret_cast<const bu::bk_span*>(base + tab_at),
                                             reinterpret_cast<const uint8_t*>(base + tab_at + (size_t)n_nodes * sizeof(bu::bk_span)), n_nodes, reinterpret_cast<uint32_t*>(base), 1));
    if (!fetch(ctx, h_records, base + rec_at, (size_t)n_nodes * sizeof(bu_tsvq_split))) return 0;
    return 1;
}

int bu_hip_tsvq_read_members(bu_hip_context* ctx, bu_tsvq* q, uint32_t buf, uint32_t start, uint32_t count, uint32_t* h_out) {
    if (!ctx || !q || buf >= bu::TSVQ_BUFS || (uint64_t)start + count > q->n) return 0;
    device_guard g(ctx->device);
    if (count) BU_TRY(ctx, d2h_pageable(ctx, h_out, q->perm[0] + (size_t)buf * q->n + start, (size_t)count * 4));
    BU_TRY(ctx, stream_wait(ctx, ctx->stream));
    return 1;
}
} // extern "C"
