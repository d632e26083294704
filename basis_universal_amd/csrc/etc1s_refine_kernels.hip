// etc1s_refine_kernels.hip -- a10: refine_endpoint_clusterization, on the lists as they come and on pre-sorted lists. Design rules of the ETC1S kernels: etc1s_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "etc1s_device.h"
#include "etc1s_kernels.h"
#include "launch_dispatch.h"

namespace bu {

// -------------------------------------------------------------------------------------------------------------------
// a10: refine_endpoint_clusterization (frontend.cpp:1772-1917)
//
// One wave per block; lanes sweep the candidate endpoint clusters (the block's parent-cluster list, or all clusters for flat
// codebooks). The block's 16 pixels are wave-uniform, the candidate's four colours are per lane. Winner = first minimum in
// list order, except that the block's current cluster wins ties at non-zero error, and a zero-error candidate ends the
// reference's scan (:1896-1904) -- encoded below from (min key, error of the current cluster).
// -------------------------------------------------------------------------------------------------------------------

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_refine_endpoint_clusterization(
    const uint4* __restrict__ pixel_blocks, uint32_t n_blocks, const uint32_t* __restrict__ block_cluster,
    const uint32_t* __restrict__ cluster_params, uint32_t n_clusters, uint32_t n_parents,
    const uint32_t* __restrict__ cand_offsets, const uint32_t* __restrict__ cand_indices, const uint8_t* __restrict__ block_parent,
    uint32_t* __restrict__ out_best) {
    constexpr uint32_t RQ = 256;   // candidates per round
    __shared__ uint2 s_q[4][2][RQ];   // per wave: {cluster parameters, position in the list | "is the block's current cluster" << 31}
    __shared__ uint32_t s_qp[4][2][RQ];   // the partial error of a candidate that survived the first four pixels
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));   // wave-uniform, and told so (see k_refine_sorted)
    if (block >= n_blocks) return; // whole wave exits together

    cvec pc[16];
    {
        const uint4* src = pixel_blocks + (size_t)block * 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = src[i];
            pc[i * 4 + 0] = pixel_cvec<PERCEPTUAL>(v.x); pc[i * 4 + 1] = pixel_cvec<PERCEPTUAL>(v.y);
            pc[i * 4 + 2] = pixel_cvec<PERCEPTUAL>(v.z); pc[i * 4 + 3] = pixel_cvec<PERCEPTUAL>(v.w);
        }
    }
    const uint32_t cur = block_cluster[block];
    const uint32_t cur_inten = (cluster_params[cur] >> 24) & 255u;

    uint32_t first = 0, total = n_clusters;
    if (n_parents) {
        const uint32_t p = block_parent[block];
        first = cand_offsets[p];
        total = cand_offsets[p + 1] - first;
    }

    // key = error << 32 | position in list; the skipped / out-of-range sentinel sorts last
    uint64_t best_key = ~0ull;
    uint32_t cur_err = 0xFFFFFFFFu;
    // The list is taken RQ candidates at a time. Each round first sorts its admissible candidates into two queues in LDS -- those whose
    // four colours need no clamping and the others -- so that the lanes are full in both sweeps (the intensity filter of :1811-1815
    // otherwise leaves holes) and the unclamped ones take the short form of the distance (etc1s_device.h, base_unclamped). The position
    // in the list travels with the candidate: the winner does not depend on the order of evaluation.
    // Pruning (exact): a candidate whose error exceeds the error of ANY member of the list can neither win nor tie. The block's current
    // cluster is a member of its own parent's list by construction, so its error -- computed here directly, one pixel per lane -- is the
    // first threshold, tightened by the running minimum after every sweep. Each sweep first takes four of the sixteen pixels (a partial
    // sum is a lower bound of the error), squeezes out the candidates that are already above the threshold, and finishes the others.
    // Should the current cluster not turn up in the list after all, everything is done again without a threshold.
    uint2 (*q)[RQ] = s_q[threadIdx.x >> 6];
    uint32_t (*qp)[RQ] = s_qp[threadIdx.x >> 6];
    uint32_t thr;
    {
        const uint32_t prm = cluster_params[cur];
        cvec bc[4];
        block_cvecs<PERCEPTUAL>(bc, scale5((int)(prm & 255u)), scale5((int)((prm >> 8) & 255u)), scale5((int)((prm >> 16) & 255u)), (int)((prm >> 24) & 7u));
        const uint32_t w = reinterpret_cast<const uint32_t*>(pixel_blocks + (size_t)block * 4)[lane & 15u];
        uint32_t e = lane < 16 ? min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(w), bc) : 0u;
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) e += (uint32_t)__shfl_xor((int)e, o, 64);
        thr = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    }
    constexpr int FIRST_PX[4] = { 0, 5, 10, 15 };
    constexpr uint64_t REST_PX = 0xEDCB98764321ull;   // the other twelve pixel indices, one per nibble
    const uint32_t* block_words = reinterpret_cast<const uint32_t*>(pixel_blocks + (size_t)block * 4);
    auto sync_queue = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto tighten = [&]() {
        uint32_t m = (uint32_t)(best_key >> 32);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o, 64));
        thr = min(thr, m);
    };
    bool seen_cur = false;
    for (int attempt = 0; attempt < 2; attempt++) {
    for (uint32_t base = 0; base < total; base += RQ) {
        uint32_t n0 = 0, n1 = 0;
#pragma unroll
        for (int i = 0; i < (int)(RQ / 64); i++) {
            const uint32_t k = base + (uint32_t)i * 64u + lane;
            bool take = k < total;
            uint32_t prm = 0, ci = 0;
            if (take) {
                ci = n_parents ? cand_indices[first + k] : k;
                prm = cluster_params[ci];
                take = ((prm >> 24) & 255u) <= cur_inten; // frontend.cpp:1811-1815
            }
            const bool plain = PERCEPTUAL && base_unclamped(scale5((int)(prm & 255u)), scale5((int)((prm >> 8) & 255u)), scale5((int)((prm >> 16) & 255u)), (int)((prm >> 24) & 7u));
            const uint64_t m0 = __ballot(take && plain), m1 = __ballot(take && !plain);
            const uint32_t r0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
            const uint32_t r1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
            const uint2 e = make_uint2(prm, k | (ci == cur ? 0x80000000u : 0u));
            if (take && plain) q[0][n0 + r0] = e;
            if (take && !plain) q[1][n1 + r1] = e;
            n0 += (uint32_t)__popcll(m0); n1 += (uint32_t)__popcll(m1);
            seen_cur = seen_cur || __ballot(take && ci == cur) != 0ull;
        }
        sync_queue();
        // ---- unclamped: one chroma term per pixel, the luma term's minimum over the four offsets
        {
            uint32_t ns = 0;
            for (uint32_t j0 = 0; j0 < n0; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool have = j < n0;
                const uint2 e = q[0][have ? j : 0];
                const int inten = (int)((e.x >> 24) & 7u);
                const cvec bcv = to_cvec<true>(scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)));
                const int a64 = k_inten_a[inten] * 64, b64 = k_inten_b[inten] * 64;
                uint32_t part = 0;
#pragma unroll
                for (int f = 0; f < 4; f++) { const int p = FIRST_PX[f]; part += min_luma_term(pc[p].x - bcv.x, a64, b64) + chroma_term(pc[p].y - bcv.y, pc[p].z - bcv.z); }
                const bool keep = have && part <= thr;
                const uint64_t m = __ballot(keep);
                const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (keep) { q[0][ns + r] = e; qp[0][ns + r] = part; }   // in place: everything up to j0 + 63 has been read
                ns += (uint32_t)__popcll(m);
            }
            sync_queue();
            // the twelve remaining pixels of a survivor are shared by four lanes (three pixels each, fetched by index: the wave-uniform
            // copy in pc[] cannot be indexed per lane), so that a handful of survivors still fills the wave
            for (uint32_t j4 = lane; j4 < ((ns * 4u + 63u) & ~63u); j4 += 64) {
                const uint32_t j = j4 >> 2, part = j4 & 3u;
                const bool have = j < ns;
                const uint2 e = q[0][have ? j : 0];
                const int inten = (int)((e.x >> 24) & 7u);
                const cvec bcv = to_cvec<true>(scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)));
                const int a64 = k_inten_a[inten] * 64, b64 = k_inten_b[inten] * 64;
                uint32_t tot = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const cvec p = pixel_cvec<true>(block_words[(REST_PX >> (4u * (part * 3u + (uint32_t)i))) & 15u]);
                    tot += min_luma_term(p.x - bcv.x, a64, b64) + chroma_term(p.y - bcv.y, p.z - bcv.z);
                }
                tot += (uint32_t)__shfl_xor((int)tot, 1, 64);
                tot += (uint32_t)__shfl_xor((int)tot, 2, 64);
                if (have && part == 0) {
                    tot += qp[0][j];
                    best_key = min(best_key, ((uint64_t)tot << 32) | (e.y & 0x7fffffffu));
                    if (e.y >> 31) cur_err = tot;
                }
            }
            if (attempt == 0) tighten();
        }
        // ---- clamped colours: the four distances
        {
            uint32_t ns = 0;
            for (uint32_t j0 = 0; j0 < n1; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool have = j < n1;
                const uint2 e = q[1][have ? j : 0];
                cvec bc[4];
                block_cvecs<PERCEPTUAL>(bc, scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)), (int)((e.x >> 24) & 7u));
                uint32_t part = 0;
#pragma unroll
                for (int f = 0; f < 4; f++) part += min_err4<PERCEPTUAL>(pc[FIRST_PX[f]], bc);
                const bool keep = have && part <= thr;
                const uint64_t m = __ballot(keep);
                const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (keep) { q[1][ns + r] = e; qp[1][ns + r] = part; }
                ns += (uint32_t)__popcll(m);
            }
            sync_queue();
            for (uint32_t j4 = lane; j4 < ((ns * 4u + 63u) & ~63u); j4 += 64) {
                const uint32_t j = j4 >> 2, part = j4 & 3u;
                const bool have = j < ns;
                const uint2 e = q[1][have ? j : 0];
                cvec bc[4];
                block_cvecs<PERCEPTUAL>(bc, scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)), (int)((e.x >> 24) & 7u));
                uint32_t tot = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) tot += min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(block_words[(REST_PX >> (4u * (part * 3u + (uint32_t)i))) & 15u]), bc);
                tot += (uint32_t)__shfl_xor((int)tot, 1, 64);
                tot += (uint32_t)__shfl_xor((int)tot, 2, 64);
                if (have && part == 0) {
                    tot += qp[1][j];
                    best_key = min(best_key, ((uint64_t)tot << 32) | (e.y & 0x7fffffffu));
                    if (e.y >> 31) cur_err = tot;
                }
            }
            if (attempt == 0) tighten();
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (seen_cur || attempt == 1) break;
    thr = 0xFFFFFFFFu; best_key = ~0ull; cur_err = 0xFFFFFFFFu;   // (not expected) the threshold was not a member's error: no pruning
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best_key, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best_key >> 32), o, 64);
        best_key = min(best_key, ((uint64_t)hi << 32) | lo);
        cur_err = min(cur_err, (uint32_t)__shfl_xor((int)cur_err, o, 64));
    }
    if (lane == 0) {
        const uint32_t min_err = (uint32_t)(best_key >> 32);
        const uint32_t k = (uint32_t)best_key;
        uint32_t winner;
        if (best_key == ~0ull) winner = 0;                       // no admissible candidate: best_cluster_index stays 0 (:1787)
        else if (min_err != 0 && cur_err == min_err) winner = cur; // tie goes to the current cluster
        else winner = n_parents ? cand_indices[first + k] : k;
        out_best[block] = winner;
    }
}

// -------------------------------------------------------------------------------------------------------------------
// a10 with pre-sorted candidate lists. k_refine_endpoint_clusterization spends a third of its instructions on finding out which of a
// list's entries a block may take at all (frontend.cpp:1811-1815: intensity table <= the block's) and which distance form they need.
// Both are properties of the (list, entry) pair, not of the block: k_refine_sort_lists (one workgroup per list, a counting sort over
// 2 classes x 8 tables in LDS) rewrites every list as [unclamped, by table][clamped, by table] with the entry's cluster parameters, its
// position in the ORIGINAL list (the tie-break key: the order of evaluation does not matter) and its cluster id, plus the 2 x 8
// cumulative counts. A block then sweeps two prefixes of that, straight from memory. Same pruning as above.
// -------------------------------------------------------------------------------------------------------------------

constexpr uint32_t RS_SEG = 18;   // per list: first entry, unclamped total, 8 cumulative unclamped counts (table <= t), 8 cumulative clamped counts

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_refine_sort_lists(const uint32_t* __restrict__ cluster_params, uint32_t n_clusters, uint32_t n_parents,
                                                           const uint32_t* __restrict__ cand_offsets, const uint32_t* __restrict__ cand_indices,
                                                           uint2* __restrict__ items, uint32_t* __restrict__ seg) {
    __shared__ uint32_t s_cnt[16], s_pos[16];
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    uint32_t first = 0, total = n_clusters;
    if (n_parents) { first = cand_offsets[p]; total = cand_offsets[p + 1] - first; }
    if (tid < 16) s_cnt[tid] = 0;
    __syncthreads();
    auto bucket_of = [&](uint32_t prm) -> uint32_t {
        const uint32_t inten = (prm >> 24) & 7u;
        const bool plain = PERCEPTUAL && base_unclamped(scale5((int)(prm & 255u)), scale5((int)((prm >> 8) & 255u)), scale5((int)((prm >> 16) & 255u)), (int)inten);
        return (plain ? 0u : 8u) + inten;
    };
    for (uint32_t k = tid; k < total; k += 256) {
        const uint32_t ci = n_parents ? cand_indices[first + k] : k;
        atomicAdd(&s_cnt[bucket_of(cluster_params[ci])], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        uint32_t* sg = seg + (size_t)p * RS_SEG;
        sg[0] = first;
        for (int b = 0; b < 16; b++) {
            s_pos[b] = run; run += s_cnt[b];
            if (b < 8) sg[2 + b] = run;                 // unclamped entries with table <= b
            else sg[10 + (b - 8)] = run - sg[9];       // clamped entries with table <= b - 8
            if (b == 7) sg[1] = run;
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < total; k += 256) {
        const uint32_t ci = n_parents ? cand_indices[first + k] : k;
        const uint32_t prm = cluster_params[ci];
        const uint32_t at = atomicAdd(&s_pos[bucket_of(prm)], 1u);
        items[first + at] = make_uint2(prm, (k << 16) | ci);   // position above the cluster id: the key order is (error, position); both fit 16 bits (caller)
    }
}

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_refine_sorted(const uint4* __restrict__ pixel_blocks, uint32_t n_blocks, const uint32_t* __restrict__ block_cluster,
                                                       const uint32_t* __restrict__ cluster_params, uint32_t n_parents, const uint2* __restrict__ items,
                                                       const uint32_t* __restrict__ seg, const uint8_t* __restrict__ block_parent, uint32_t* __restrict__ out_best) {
    constexpr uint32_t RQ = 256;
    __shared__ uint2 s_q[4][RQ];        // per wave: the survivors of a sweep's first four pixels
    __shared__ uint32_t s_qp[4][RQ];    // and their partial errors
    const uint32_t lane = threadIdx.x & 63u;
    // (wave-uniform, and told so: the block's tile is then fetched with scalar loads and its sixteen colour vectors are made on the scalar unit, once per wave instead of per lane)
    const uint32_t block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (block >= n_blocks) return; // whole wave exits together

    cvec pc[16];
    {
        const uint4* src = pixel_blocks + (size_t)block * 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = src[i];
            pc[i * 4 + 0] = pixel_cvec<PERCEPTUAL>(v.x); pc[i * 4 + 1] = pixel_cvec<PERCEPTUAL>(v.y);
            pc[i * 4 + 2] = pixel_cvec<PERCEPTUAL>(v.z); pc[i * 4 + 3] = pixel_cvec<PERCEPTUAL>(v.w);
        }
    }
    // the tile's chroma moments (wave-uniform: scalar unit): what the sweep's first look at an unclamped candidate bounds its sixteen chroma terms with
    chroma_moments cm = { 0, 0, 0, 0, 0, 0 };
    if (PERCEPTUAL) {
        int s1y = 0, s1z = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { s1y += pc[i].y; s1z += pc[i].z; }
        cm.my = s1y >> 4; cm.mz = s1z >> 4; cm.r1y = s1y - 16 * cm.my; cm.r1z = s1z - 16 * cm.mz;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int ry = pc[i].y - cm.my, rz = pc[i].z - cm.mz;
            cm.r2y += (int)((uint32_t)(ry * ry) >> 10); cm.r2z += (int)((uint32_t)(rz * rz) >> 10);
        }
    }
    const uint32_t cur = block_cluster[block];
    const uint32_t cur_prm = cluster_params[cur];
    const uint32_t cur_inten = (cur_prm >> 24) & 7u;
    const uint32_t* sg = seg + (size_t)(n_parents ? block_parent[block] : 0u) * RS_SEG;
    const uint32_t first = sg[0], plain_total = sg[1];
    const uint32_t n_plain = sg[2 + cur_inten], n_clamped = sg[10 + cur_inten];
    const uint2* plain_items = items + first;
    const uint2* clamped_items = items + first + plain_total;

    constexpr uint64_t REST_PX = 0xEDCB98764321ull;   // the other twelve pixel indices, one per nibble
    const uint32_t* block_words = reinterpret_cast<const uint32_t*>(pixel_blocks + (size_t)block * 4);
    uint2* q = s_q[threadIdx.x >> 6];
    uint32_t* qp = s_qp[threadIdx.x >> 6];
    uint64_t best_key = ~0ull;
    uint32_t cur_err = 0xFFFFFFFFu;
    uint32_t thr;   // the error of the block's own cluster (a list member by construction), see k_refine_endpoint_clusterization
    {
        const int cr = scale5((int)(cur_prm & 255u)), cg = scale5((int)((cur_prm >> 8) & 255u)), cb = scale5((int)((cur_prm >> 16) & 255u));
        uint32_t e = 0;
        if (PERCEPTUAL && base_unclamped(cr, cg, cb, (int)cur_inten)) {   // (wave-uniform) nine clusters in ten: one chroma term and two squares instead of four distances
            const cvec bcv = to_cvec<true>(cr, cg, cb);
            const cvec p = pixel_cvec<true>(block_words[lane & 15u]);
            if (lane < 16) e = min_luma_term(p.x - bcv.x, k_inten_a[cur_inten] * 64, k_inten_b[cur_inten] * 64) + chroma_term(p.y - bcv.y, p.z - bcv.z);
        } else {
            cvec bc[4];
            block_cvecs<PERCEPTUAL>(bc, cr, cg, cb, (int)cur_inten);
            if (lane < 16) e = min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(block_words[lane & 15u]), bc);
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) e += (uint32_t)__shfl_xor((int)e, o, 64);
        thr = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    }
    auto sync_queue = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto tighten = [&]() {
        uint32_t m = (uint32_t)(best_key >> 32);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o, 64));
        thr = min(thr, m);
    };
    bool seen_cur = false;
    for (int attempt = 0; attempt < 2; attempt++) {
        // ---- unclamped: one chroma term per pixel, the luma term's minimum over the four offsets
        for (uint32_t base = 0; base < n_plain; base += RQ) {
            const uint32_t n0 = min(RQ, n_plain - base);
            uint32_t ns = 0;
            for (uint32_t j0 = 0; j0 < n0; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool have = j < n0;
                const uint2 e = plain_items[base + (have ? j : 0)];
                const cvec bcv = to_cvec<true>(scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)));
                // a lower bound of the candidate's error: a bound of all sixteen chroma terms from the tile's moments (chroma_lower_bound: 20 instructions, and it sees the whole
                // tile). Luma terms of a few pixels on top of it were measured and cost more than they prune: with 4 / 2 / 0 pixels' luma terms the kernel takes 1.64 / 1.59 / 1.52 ms
                // (8192^2 q255: 9.2 / 8.4 / 7.8), and a bound from the tile's luma range 1.57 -- the chroma bound decides
                const uint32_t part = chroma_lower_bound(cm, bcv.y, bcv.z);
                const bool keep = have && part <= thr;
                const uint64_t m = __ballot(keep);
                const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (keep) q[ns + r] = e;
                ns += (uint32_t)__popcll(m);
                seen_cur = seen_cur || __ballot(have && (e.y & 0xffffu) == cur) != 0ull;
            }
            sync_queue();
            for (uint32_t j4 = lane; j4 < ((ns * 4u + 63u) & ~63u); j4 += 64) {   // four lanes per survivor, four pixels each: the exact error
                const uint32_t j = j4 >> 2, part = j4 & 3u;
                const bool have = j < ns;
                const uint2 e = q[have ? j : 0];
                const int inten = (int)((e.x >> 24) & 7u);
                const cvec bcv = to_cvec<true>(scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)));
                const int a64 = k_inten_a[inten] * 64, b64 = k_inten_b[inten] * 64;
                uint32_t tot = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const cvec p = pixel_cvec<true>(block_words[part * 4u + (uint32_t)i]);
                    tot += min_luma_term(p.x - bcv.x, a64, b64) + chroma_term(p.y - bcv.y, p.z - bcv.z);
                }
                tot += (uint32_t)__shfl_xor((int)tot, 1, 64);
                tot += (uint32_t)__shfl_xor((int)tot, 2, 64);
                if (have && part == 0) {
                    best_key = min(best_key, ((uint64_t)tot << 32) | e.y);
                    if ((e.y & 0xffffu) == cur) cur_err = tot;
                }
            }
            if (attempt == 0) tighten();
            __builtin_amdgcn_wave_barrier();
        }
        // ---- clamped colours: the four distances
        for (uint32_t base = 0; base < n_clamped; base += RQ) {
            const uint32_t n1 = min(RQ, n_clamped - base);
            uint32_t ns = 0;
            // the clamped entries are few (a tenth of a list on the bench image) and need the expensive four-distance form: FOUR lanes per entry
            // take one of the four test pixels each (pixel 5 f), so that a handful of entries costs one pass of one distance instead of one of four
            for (uint32_t j0 = 0; j0 < n1; j0 += 16) {
                const uint32_t j = j0 + (lane >> 2), f = lane & 3u;
                const bool have = j < n1;
                const uint2 e = clamped_items[base + (have ? j : 0)];
                cvec bc[4];
                block_cvecs<PERCEPTUAL>(bc, scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)), (int)((e.x >> 24) & 7u));
                uint32_t part = min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(block_words[f * 5u]), bc);   // FIRST_PX[f] = 5 f
                part += (uint32_t)__shfl_xor((int)part, 1, 64);
                part += (uint32_t)__shfl_xor((int)part, 2, 64);
                const bool keep = have && f == 0 && part <= thr;
                const uint64_t m = __ballot(keep);
                const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (keep) { q[ns + r] = e; qp[ns + r] = part; }
                ns += (uint32_t)__popcll(m);
                seen_cur = seen_cur || __ballot(have && (e.y & 0xffffu) == cur) != 0ull;
            }
            sync_queue();
            for (uint32_t j4 = lane; j4 < ((ns * 4u + 63u) & ~63u); j4 += 64) {
                const uint32_t j = j4 >> 2, part = j4 & 3u;
                const bool have = j < ns;
                const uint2 e = q[have ? j : 0];
                cvec bc[4];
                block_cvecs<PERCEPTUAL>(bc, scale5((int)(e.x & 255u)), scale5((int)((e.x >> 8) & 255u)), scale5((int)((e.x >> 16) & 255u)), (int)((e.x >> 24) & 7u));
                uint32_t tot = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) tot += min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(block_words[(REST_PX >> (4u * (part * 3u + (uint32_t)i))) & 15u]), bc);
                tot += (uint32_t)__shfl_xor((int)tot, 1, 64);
                tot += (uint32_t)__shfl_xor((int)tot, 2, 64);
                if (have && part == 0) {
                    tot += qp[j];
                    best_key = min(best_key, ((uint64_t)tot << 32) | e.y);
                    if ((e.y & 0xffffu) == cur) cur_err = tot;
                }
            }
            if (attempt == 0) tighten();
            __builtin_amdgcn_wave_barrier();
        }
        if (seen_cur || attempt == 1) break;
        thr = 0xFFFFFFFFu; best_key = ~0ull; cur_err = 0xFFFFFFFFu;   // (not expected) the threshold was not a member's error: no pruning
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best_key, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best_key >> 32), o, 64);
        best_key = min(best_key, ((uint64_t)hi << 32) | lo);
        cur_err = min(cur_err, (uint32_t)__shfl_xor((int)cur_err, o, 64));
    }
    if (lane == 0) {
        const uint32_t min_err = (uint32_t)(best_key >> 32);
        uint32_t winner;
        if (best_key == ~0ull) winner = 0;                       // no admissible candidate: best_cluster_index stays 0 (:1787)
        else if (min_err != 0 && cur_err == min_err) winner = cur; // tie goes to the current cluster
        else winner = (uint32_t)best_key & 0xffffu;                // the winning entry's cluster id rides below its position
        out_best[block] = winner;
    }
}

static size_t refine_items_bytes(uint32_t n_clusters, size_t lists) { return (lists * n_clusters * sizeof(uint2) + 255) & ~(size_t)255; }   // a cluster is at most once in a list

size_t refine_workspace_bytes(uint32_t n_clusters, uint32_t n_parents) {
    if (n_clusters > 65535u) return 0;   // positions and cluster ids share a dword in the sorted lists
    const size_t lists = n_parents ? n_parents : 1;
    return refine_items_bytes(n_clusters, lists) + lists * RS_SEG * sizeof(uint32_t);
}

hipError_t launch_refine_endpoint_clusterization(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint32_t* d_block_cluster,
                                                 const uint8_t* d_cluster_params, uint32_t n_clusters, uint32_t n_parents, const uint32_t* d_cand_offsets,
                                                 const uint32_t* d_cand_indices, const uint8_t* d_block_parent, bool perceptual, uint32_t* d_out_best, void* d_work) {
    if (!n_blocks) return hipSuccess;
    const dim3 grid((n_blocks + 3) / 4), blk(256);
    const uint4* in = static_cast<const uint4*>(d_pixel_blocks);
    const uint32_t* prm = reinterpret_cast<const uint32_t*>(d_cluster_params);
    const bool sorted = d_work && refine_workspace_bytes(n_clusters, n_parents);
    with_bool(perceptual, [&](auto p) {
        constexpr bool P = decltype(p)::value;
        if (sorted) {
            const size_t lists = n_parents ? n_parents : 1;
            uint2* items = static_cast<uint2*>(d_work);
            uint32_t* seg = reinterpret_cast<uint32_t*>(static_cast<char*>(d_work) + refine_items_bytes(n_clusters, lists));
            hipLaunchKernelGGL(k_refine_sort_lists<P>, dim3((uint32_t)lists), blk, 0, st, prm, n_clusters, n_parents, d_cand_offsets, d_cand_indices, items, seg);
            hipLaunchKernelGGL(k_refine_sorted<P>, grid, blk, 0, st, in, n_blocks, d_block_cluster, prm, n_parents, items, seg, d_block_parent, d_out_best);
        } else {
            hipLaunchKernelGGL(k_refine_endpoint_clusterization<P>, grid, blk, 0, st, in, n_blocks, d_block_cluster, prm, n_clusters, n_parents, d_cand_offsets, d_cand_indices,
                               d_block_parent, d_out_best);
        }
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace bu
