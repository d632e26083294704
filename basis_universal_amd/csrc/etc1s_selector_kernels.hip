// etc1s_selector_kernels.hip -- the selector side of the frontend: a11 determine_selectors, a12 the selector training vectors, a13 create_optimized_selector_codebook
// (k_cosc_*), a14 find_optimal_selector_clusters_for_each_block (k_fosc_*). Design rules of the ETC1S kernels: etc1s_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "etc1s_device.h"
#include "etc1s_kernels.h"
#include "launch_dispatch.h"

namespace bu {

// -------------------------------------------------------------------------------------------------------------------
// a12: selector training vectors (frontend.cpp:2155-2183)
// -------------------------------------------------------------------------------------------------------------------

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_selector_training_vectors(const uint64_t* __restrict__ enc_blocks, uint32_t n_blocks, float* __restrict__ out16, uint64_t* __restrict__ out_w) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    const uint64_t m = enc_blocks[i];
    uint32_t r5, g5, b5, inten;
    unpack_etc1s_header(m, r5, g5, b5, inten);
    const uint32_t lo = (uint32_t)bswap64(m);
    if (out16) { // the resident frontend only needs the weights: it de-duplicates on the packed selector word
        float4* o = reinterpret_cast<float4*>(out16 + (size_t)i * 16);
#pragma unroll
        for (uint32_t y = 0; y < 4; y++) {
            float4 v;
            v.x = (float)selector_from_bits(lo, 0, y); v.y = (float)selector_from_bits(lo, 1, y);
            v.z = (float)selector_from_bits(lo, 2, y); v.w = (float)selector_from_bits(lo, 3, y);
            o[y] = v;
        }
    }
    const int br = scale5((int)r5), bg = scale5((int)g5), bb = scale5((int)b5), d = k_inten_b[inten];
    const cvec lo_c = to_cvec<PERCEPTUAL>(clamp255(br - d), clamp255(bg - d), clamp255(bb - d));
    const cvec hi_c = to_cvec<PERCEPTUAL>(clamp255(br + d), clamp255(bg + d), clamp255(bb + d));
    const uint32_t dist = cdist<PERCEPTUAL>(lo_c, hi_c);
    out_w[i] = (uint64_t)min(max(dist / 300u, 1u), 4096u);
}

// -------------------------------------------------------------------------------------------------------------------
// a11: create_initial_packed_texture -> etc_block::determine_selectors (frontend.cpp:2058-2085, etc.h:374-436)
//
// 16 lanes per block, lane l owns pixel (x = l>>2, y = l&3) so that a wave ballot of "raw selector lsb/msb" IS the packed
// selector bit plane (bit index x*4+y). The only kernel of the path that is close to HBM-bound: 64 B in, 8 B out per block.
// -------------------------------------------------------------------------------------------------------------------

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_determine_selectors(
    const uint32_t* __restrict__ pixel_words, uint32_t n_blocks, const uint32_t* __restrict__ color5_inten,
    const uint32_t* __restrict__ block_cluster, uint2* __restrict__ out_blocks) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t block_raw = gid >> 4;
    const bool in_range = block_raw < n_blocks;
    const uint32_t block = in_range ? block_raw : (n_blocks - 1);
    const uint32_t l = threadIdx.x & 15u;
    const uint32_t x = l >> 2, y = l & 3u;
    const uint32_t w = pixel_words[(size_t)block * 16 + y * 4 + x];
    const uint32_t prm = block_cluster ? color5_inten[block_cluster[block]] : color5_inten[block];
    const uint32_t inten = (prm >> 24) & 255u;
    cvec bc[4];
    block_cvecs<PERCEPTUAL>(bc, scale5((int)(prm & 255u)), scale5((int)((prm >> 8) & 255u)), scale5((int)((prm >> 16) & 255u)), (int)inten);
    const uint32_t s = best_sel4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(w), bc);
    const uint32_t raw = (0x4Bu >> (s * 2)) & 3u;
    const uint64_t lsb = __ballot(raw & 1u);
    const uint64_t msb = __ballot(raw >> 1);
    const uint32_t group = (threadIdx.x & 63u) >> 4;
    if (l == 0 && in_range) {
        const uint32_t bits = (uint32_t)((lsb >> (group * 16)) & 0xFFFFu) | ((uint32_t)((msb >> (group * 16)) & 0xFFFFu) << 16);
        const uint64_t v = etc1s_header_bits(prm & 255u, (prm >> 8) & 255u, (prm >> 16) & 255u, inten) | bits;
        const uint64_t m = bswap64(v);
        out_blocks[block] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
}

// -------------------------------------------------------------------------------------------------------------------
// a13: create_optimized_selector_codebook (frontend.cpp:2259-2354)
//
// lane = (pixel p = lane>>2, selector s = lane&3) accumulates the u64 error of "pixel p of every member block encoded with selector s" --
// exactly the reference's total_err[y][x][s] -- then a 4-lane first-min picks the pixel's selector. Clusters are very uneven (a few hold tens
// of thousands of blocks), so the accumulation is cut by POSITION in the CSR member array, not by cluster: every wave takes COSC_CHUNK
// consecutive members, finds the cluster its first member belongs to (binary search in the offsets) and walks on, flushing its partial sums
// into the cluster's 64 u64 counters with atomic adds whenever it crosses into the next cluster. Integer sums: exact in any order. A second
// kernel (one wave per cluster) turns the counters into selectors.
// -------------------------------------------------------------------------------------------------------------------

constexpr uint32_t COSC_CHUNK = 128;
constexpr uint32_t COSC_WORKGROUPS = 2048;   // of four waves: one chunk per wave for a 4096^2 image, the waves stride over the chunks of a larger one

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_cosc_accumulate(
    const uint32_t* __restrict__ pixel_words, const uint64_t* __restrict__ enc_blocks, uint32_t n_clusters,
    const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ block_indices, unsigned long long* __restrict__ acc) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));   // wave-uniform, and told so: the search below runs on the scalar unit
    // (the launch is a fixed number of waves that stride over the chunks: how many members the offsets span is on the device only, and asking for it was a round trip)
    const uint32_t begin = offsets[0], end = offsets[n_clusters];
    for (uint64_t lo64 = (uint64_t)begin + (uint64_t)wave * COSC_CHUNK; lo64 < end; lo64 += (uint64_t)gridDim.x * 4u * COSC_CHUNK) {
    const uint32_t lo = (uint32_t)lo64, hi = end - lo > COSC_CHUNK ? lo + COSC_CHUNK : end;
    // cluster of member `lo`: the last cluster whose first member is <= lo (empty clusters in front of it share that offset and are skipped)
    uint32_t a = 0, b = n_clusters;  // invariant: offsets[a] <= lo < offsets[b]
    while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (offsets[m] <= lo) a = m; else b = m; }
    uint32_t ci = a, next = offsets[ci + 1];
    const uint32_t p = lane >> 2, s = lane & 3u;
    unsigned long long tot = 0;
    for (uint32_t k = lo; k < hi; k++) {
        while (k >= next) {  // crossed into the next (non-empty) cluster
            if (tot) atomicAdd(&acc[(size_t)ci * 64 + lane], tot);
            tot = 0;
            ci++; next = offsets[ci + 1];
        }
        const uint32_t bi = block_indices[k];
        uint32_t r5, g5, b5, inten;
        unpack_etc1s_header(enc_blocks[bi], r5, g5, b5, inten);
        const int yd = inten_delta((int)inten, (int)s);
        const cvec c = to_cvec<PERCEPTUAL>(clamp255(scale5((int)r5) + yd), clamp255(scale5((int)g5) + yd), clamp255(scale5((int)b5) + yd));
        tot += cdist<PERCEPTUAL>(c, pixel_cvec<PERCEPTUAL>(pixel_words[(size_t)bi * 16 + p]));
    }
    if (tot) atomicAdd(&acc[(size_t)ci * 64 + lane], tot);
    }
}

__global__ __launch_bounds__(256) void k_cosc_select(uint32_t n_clusters, const uint32_t* __restrict__ offsets, const unsigned long long* __restrict__ acc,
                                                     uint64_t* __restrict__ selector_blocks) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ci = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ci >= n_clusters) return;
    if (offsets[ci + 1] == offsets[ci]) return; // empty clusters keep their previous selectors (frontend.cpp:2282-2283)
    const uint32_t p = lane >> 2, s = lane & 3u;
    // first-min over the 4 selectors of this pixel: compare (tot, s) lexicographically
    uint64_t bt = acc[(size_t)ci * 64 + lane]; uint32_t bs = s;
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bt, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(bt >> 32), o, 64);
        const uint64_t ot = ((uint64_t)hi << 32) | lo;
        const uint32_t os = (uint32_t)__shfl_xor((int)bs, o, 64);
        if (ot < bt || (ot == bt && os < bs)) { bt = ot; bs = os; }
    }
    // pixel p = y*4+x
    uint32_t bits = (s == 0) ? selector_bits(p & 3u, p >> 2, bs) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o, 64);
    if (lane == 0) {
        const uint64_t v = (bswap64(selector_blocks[ci]) & ~0xFFFFFFFFull) | bits;
        selector_blocks[ci] = bswap64(v);
    }
}

// -------------------------------------------------------------------------------------------------------------------
// a14: find_optimal_selector_clusters_for_each_block (frontend.cpp:2534-2706)
//
// One wave per block. The 4x16 table err[s][p] of the block's endpoint is built by the 64 lanes (one entry each) into LDS;
// lanes then sweep candidate codebook entries, summing 16 table lookups each (all lanes of a step hit one of 4 banks per
// pixel -> conflict-free broadcasts). Winner = first minimum in list order; the reference's early-outs (:2640-2660) never
// change it. The "identical to the previous block of this 2048-block job" shortcut (:2557-2564) is applied by a second
// pass so that results stay identical even when equal tiles carry different endpoints.
// -------------------------------------------------------------------------------------------------------------------

// A candidate's error is a sum of 16 table entries err[selector of texel][texel]. The selector word keeps texel i's two bits at positions i and 16 + i (i = x * 4 + y), so two
// neighbouring texels' selectors are a 4-bit code (two low-plane bits, two high-plane bits) and their two entries one entry of a 16-entry PAIR table: 8 look-ups per candidate
// instead of 16, after 128 entries built once per block by the wave (integer sums: any grouping gives the same total). Blocks offered many candidates (q255: ~1,000 per block)
// go one step further, four texels = an 8-bit code into four 256-entry tables made from the pair tables: 4 look-ups per candidate.
// the low 32 bits (the selector bits) of every candidate in list order: words[j] = bits of selector_blocks[cand_indices[j]] (flat codebook: of selector_blocks[j])
__global__ __launch_bounds__(256) void k_fosc_candidate_words(const uint64_t* __restrict__ selector_blocks, uint32_t n_selectors, uint32_t n_parents,
                                                              const uint32_t* __restrict__ cand_offsets, const uint32_t* __restrict__ cand_indices, uint32_t* __restrict__ words) {
    const uint32_t total = n_parents ? cand_offsets[n_parents] : n_selectors;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < total; j += gridDim.x * 256u)
        words[j] = (uint32_t)bswap64(selector_blocks[n_parents ? cand_indices[j] : j]);
}

constexpr uint32_t FOSC_QUAD_MIN = 384;   // candidates per block from which the 1,024-entry tables pay for themselves (16 entries per lane to build)

template <bool PERCEPTUAL>
__global__ __launch_bounds__(256) void k_find_optimal_selector_clusters(
    const uint32_t* __restrict__ pixel_words, const uint64_t* __restrict__ enc_blocks, uint32_t n_blocks,
    const uint64_t* __restrict__ selector_blocks, uint32_t n_selectors, uint32_t n_parents,
    const uint32_t* __restrict__ cand_offsets, const uint32_t* __restrict__ cand_indices, const uint8_t* __restrict__ block_parent,
    uint32_t* __restrict__ out_idx, const uint32_t* __restrict__ cand_words) {
    __shared__ uint32_t s_err[4][64];     // [wave][s*16+p]
    __shared__ uint32_t s_pair[4][128];   // [wave][g*16 + code4]: texels with selector bits 2g, 2g + 1
    __shared__ uint32_t s_quad[4][1024];  // [wave][h*256 + code8]: texels with selector bits 4h .. 4h + 3
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t block = blockIdx.x * 4u + wave;   // wave-uniform, and told so: the block's header, parent and list bounds come through scalar loads
    if (block >= n_blocks) return;

    {
        uint32_t r5, g5, b5, inten;
        unpack_etc1s_header(enc_blocks[block], r5, g5, b5, inten);
        const uint32_t s = lane >> 4, p = lane & 15u;
        const int yd = inten_delta((int)inten, (int)s);
        const cvec c = to_cvec<PERCEPTUAL>(clamp255(scale5((int)r5) + yd), clamp255(scale5((int)g5) + yd), clamp255(scale5((int)b5) + yd));
        s_err[wave][lane] = cdist<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(pixel_words[(size_t)block * 16 + p]), c);
    }
    // same-wave producer/consumer: LDS ops of one wave are ordered
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t e = 0; e < 2; e++) {
        const uint32_t idx = lane + e * 64u, g = idx >> 4, code = idx & 15u;
        const uint32_t i0 = 2u * g, i1 = i0 + 1u;                               // selector bit positions = x * 4 + y
        const uint32_t raw0 = (code & 1u) | ((code >> 1) & 2u), raw1 = ((code >> 1) & 1u) | ((code >> 2) & 2u);
        const uint32_t s0 = (0x1Eu >> (raw0 * 2)) & 3u, s1 = (0x1Eu >> (raw1 * 2)) & 3u;   // g_etc1_to_selector_index (selector_from_bits)
        const uint32_t p0 = (i0 & 3u) * 4u + (i0 >> 2), p1 = (i1 & 3u) * 4u + (i1 >> 2);   // raster texel y * 4 + x
        s_pair[wave][idx] = s_err[wave][s0 * 16 + p0] + s_err[wave][s1 * 16 + p1];
    }
    __builtin_amdgcn_wave_barrier();

    uint32_t first = 0, total = n_selectors;
    if (n_parents) {
        const uint32_t p = block_parent[block];
        first = cand_offsets[p];
        total = cand_offsets[p + 1] - first;
    }
    uint64_t best_key = ~0ull;
    if (total >= FOSC_QUAD_MIN) {   // wave-uniform
#pragma unroll
        for (uint32_t e = 0; e < 16; e++) {
            const uint32_t idx = lane + e * 64u, h = idx >> 8, code = idx & 255u, a = code & 15u, b = code >> 4;
            const uint32_t c_lo = (a & 3u) | ((b & 3u) << 2), c_hi = (a >> 2) | (b & 12u);
            s_quad[wave][idx] = s_pair[wave][(2u * h) * 16u + c_lo] + s_pair[wave][(2u * h + 1u) * 16u + c_hi];
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t k = lane; k < total; k += 64) {
            // cand_words (k_fosc_candidate_words): the candidates' selector words laid out in list order -- one coalesced load instead of list entry, then codebook entry
            uint32_t lo;
            if (cand_words) lo = cand_words[first + k];
            else { const uint32_t ci = n_parents ? cand_indices[first + k] : k; lo = (uint32_t)bswap64(selector_blocks[ci]); }
            uint32_t e = 0;
#pragma unroll
            for (uint32_t h = 0; h < 4; h++) e += s_quad[wave][h * 256u + (((lo >> (4u * h)) & 15u) | (((lo >> (16u + 4u * h)) & 15u) << 4))];
            best_key = min(best_key, ((uint64_t)e << 32) | k);
        }
    } else {
        for (uint32_t k = lane; k < total; k += 64) {
            // cand_words (k_fosc_candidate_words): the candidates' selector words laid out in list order -- one coalesced load instead of list entry, then codebook entry
            uint32_t lo;
            if (cand_words) lo = cand_words[first + k];
            else { const uint32_t ci = n_parents ? cand_indices[first + k] : k; lo = (uint32_t)bswap64(selector_blocks[ci]); }
            uint32_t e = 0;
#pragma unroll
            for (uint32_t g = 0; g < 8; g++) e += s_pair[wave][g * 16u + (((lo >> (2u * g)) & 3u) | (((lo >> (16u + 2u * g)) & 3u) << 2))];
            best_key = min(best_key, ((uint64_t)e << 32) | k);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best_key, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best_key >> 32), o, 64);
        best_key = min(best_key, ((uint64_t)hi << 32) | lo);
    }
    if (lane == 0) {
        const uint32_t k = (uint32_t)best_key;
        out_idx[block] = (best_key == ~0ull) ? 0u : (n_parents ? cand_indices[first + k] : k);
    }
}

// Pass 2 of a14: resolve runs of identical consecutive tiles inside each `chunk`-block job to the run head's choice
// (frontend.cpp:2557-2564), then stamp the chosen selector bits into the encoded blocks (:2688-2690).
__global__ __launch_bounds__(256) void k_fosc_resolve_and_stamp(
    const uint4* __restrict__ pixel_blocks, uint64_t* __restrict__ enc_blocks, uint32_t n_blocks, const uint64_t* __restrict__ selector_blocks,
    uint32_t chunk, const uint32_t* __restrict__ raw_idx, uint32_t* __restrict__ out_idx) {
    const uint32_t block = blockIdx.x * blockDim.x + threadIdx.x;
    if (block >= n_blocks) return;
    uint32_t head = block;
    if (chunk) {
        const uint32_t chunk_first = (block / chunk) * chunk;
        while (head > chunk_first) {
            const uint4* a = pixel_blocks + (size_t)head * 4;
            const uint4* b = pixel_blocks + (size_t)(head - 1) * 4;
            bool same = true;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint4 u = a[i], v = b[i];
                same = same && (u.x == v.x) && (u.y == v.y) && (u.z == v.z) && (u.w == v.w);
            }
            if (!same) break;
            head--;
        }
    }
    const uint32_t best = raw_idx[head];
    out_idx[block] = best;
    const uint64_t hdr = bswap64(enc_blocks[block]) & ~0xFFFFFFFFull;
    const uint64_t sel = bswap64(selector_blocks[best]) & 0xFFFFFFFFull;
    enc_blocks[block] = bswap64(hdr | sel);
}

// -------------------------------------------------------------------------------------------------------------------
// Launchers
// -------------------------------------------------------------------------------------------------------------------

hipError_t launch_selector_training_vectors(hipStream_t st, const void* d_enc_blocks, uint32_t n_blocks, bool perceptual, float* d_out16, uint64_t* d_w) {
    if (!n_blocks) return hipSuccess;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_selector_training_vectors<decltype(p)::value>, dim3((n_blocks + 255) / 256), dim3(256), 0, st, static_cast<const uint64_t*>(d_enc_blocks), n_blocks, d_out16, d_w);
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_determine_selectors(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint8_t* d_color5_inten,
                                      const uint32_t* d_block_cluster, bool perceptual, void* d_out) {
    if (!n_blocks) return hipSuccess;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_determine_selectors<decltype(p)::value>, dim3((n_blocks + 15) / 16), dim3(256), 0, st, static_cast<const uint32_t*>(d_pixel_blocks), n_blocks,
                           reinterpret_cast<const uint32_t*>(d_color5_inten), d_block_cluster, static_cast<uint2*>(d_out));
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

size_t create_optimized_selector_codebook_workspace_bytes(uint32_t n_clusters) { return (size_t)n_clusters * 64 * 8; }

hipError_t launch_create_optimized_selector_codebook(hipStream_t st, const void* d_pixel_blocks, const void* d_enc_blocks, uint32_t n_clusters,
                                                     const uint32_t* d_offsets, const uint32_t* d_block_indices, bool perceptual,
                                                     void* d_workspace, void* d_selector_blocks) {
    if (!n_clusters) return hipSuccess;
    unsigned long long* acc = static_cast<unsigned long long*>(d_workspace);
    hipError_t e = hipMemsetAsync(acc, 0, create_optimized_selector_codebook_workspace_bytes(n_clusters), st);
    if (e != hipSuccess) return e;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_cosc_accumulate<decltype(p)::value>, dim3(COSC_WORKGROUPS), dim3(256), 0, st, static_cast<const uint32_t*>(d_pixel_blocks),
                           static_cast<const uint64_t*>(d_enc_blocks), n_clusters, d_offsets, d_block_indices, acc);
    });
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cosc_select, dim3((n_clusters + 3) / 4), dim3(256), 0, st, n_clusters, d_offsets, acc, static_cast<uint64_t*>(d_selector_blocks));
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_find_optimal_selector_clusters(hipStream_t st, const void* d_pixel_blocks, void* d_enc_blocks, uint32_t n_blocks,
                                                 const void* d_selector_blocks, uint32_t n_selectors, uint32_t n_parents, const uint32_t* d_cand_offsets,
                                                 const uint32_t* d_cand_indices, const uint8_t* d_block_parent, bool perceptual, uint32_t chunk,
                                                 uint32_t* d_scratch_idx, uint32_t* d_out_idx, uint32_t* d_cand_words, size_t cand_words_capacity) {
    if (!n_blocks) return hipSuccess;
    const uint64_t* selectors = static_cast<const uint64_t*>(d_selector_blocks);
    // (a list holds every selector at most once: n_parents x n_selectors entries bound the lists' total, which only the device knows)
    const size_t most = (size_t)(n_parents ? n_parents : 1u) * n_selectors;
    if (d_cand_words && cand_words_capacity >= most && most) {
        hipLaunchKernelGGL(k_fosc_candidate_words, dim3((uint32_t)std::min<size_t>((most + 255) / 256, 2048)), dim3(256), 0, st, selectors, n_selectors, n_parents,
                           d_cand_offsets, d_cand_indices, d_cand_words);
        BU_LAUNCH_CHECK();
    } else d_cand_words = nullptr;
    with_bool(perceptual, [&](auto p) {
        hipLaunchKernelGGL(k_find_optimal_selector_clusters<decltype(p)::value>, dim3((n_blocks + 3) / 4), dim3(256), 0, st, static_cast<const uint32_t*>(d_pixel_blocks),
                           static_cast<const uint64_t*>(d_enc_blocks), n_blocks, selectors, n_selectors, n_parents, d_cand_offsets, d_cand_indices, d_block_parent, d_scratch_idx,
                           d_cand_words);
    });
    BU_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fosc_resolve_and_stamp, dim3((n_blocks + 255) / 256), dim3(256), 0, st, static_cast<const uint4*>(d_pixel_blocks),
                       static_cast<uint64_t*>(d_enc_blocks), n_blocks, selectors, chunk, d_scratch_idx, d_out_idx);
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace bu
