// etc1s_cluster_fit_kernels.hip -- a9: the etc1_optimizer over all texels of an endpoint cluster (generate_endpoint_codebook) and the same fit with the selectors
// held fixed (refine_block_endpoints_given_selectors, reoptimize_remapped_endpoints): one workgroup per cluster here, many per LARGE cluster in
// etc1s_codebook_wide.inc. Design rules of the ETC1S kernels: etc1s_kernels.h.
#include "etc1s_fit_common.h"
#include "launch_dispatch.h"

namespace bu {

hipError_t upload_cluster_fit_tables() { return upload_fit_tables(); }

// -------------------------------------------------------------------------------------------------------------------
// a9: generate_endpoint_codebook (frontend.cpp:1482-1613) -- etc1_optimizer over all pixels of an endpoint cluster.
//
// One 1024-thread workgroup per cluster (largest clusters are dispatched first). A trial is one pass over the cluster's
// pixels computing all 8 intensity-table totals at once (u64), a wave shuffle reduction and a 16-wave LDS reduction.
// Pixels are gathered straight from the resident tiles: training vector v = block*2+subblock owns the 32 contiguous
// bytes of rows 2*subblock..2*subblock+1 (flipped layout, etc.cpp:352-361).
// The float colour mean is order dependent beyond 2^24 (SURVEY hazard H4): integer channel sums <= 2^24 are provably
// identical to the reference's running float sum; otherwise three lanes replay the float accumulation in pixel order.
// -------------------------------------------------------------------------------------------------------------------

constexpr int CB_THREADS = 512;   // 1024 leaves the SIMDs 44 % idle on the bench image (barriers per trial, ~7 pixels per thread); 512: 1.14 ms against 1.80
constexpr int CB_WAVES = CB_THREADS / 64;
// The first CB_STAGE texels of a cluster are kept in LDS after the first pass over them: every trial (17 at the default quality, up to 166) re-reads the
// cluster's texels, and from memory that is two dependent loads per texel (member list, then the tile) -- 7.7x the algorithmic bytes fetched per launch in
// round 2's FETCH_SIZE pass. 8192 texels (32 KiB) hold the whole cluster for all but the largest few; the rest of a larger cluster still comes from L2.
constexpr uint32_t CB_STAGE = 8192;

// xor butterfly: EVERY lane ends up with the wave's total (tsvq_common.h has a wave_sum_u64 of its own: a DPP prefix sum whose total only lane 63 holds)
__device__ __forceinline__ uint64_t wave_allsum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t cluster_pixel(const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ members, uint32_t j) {
    const uint32_t tv = members[j >> 3];
    // word index = block*16 + subblock*8 + (j & 7); tv = block*2 + subblock
    return pixel_words[(size_t)tv * 8 + (j & 7u)];
}

// forced selector of cluster pixel j (refine_block_endpoints_given_selectors, frontend.cpp:2766-2775): the selector the block's
// current encoding gives that texel; sub-block texels are the flipped layout, i.e. rows {0,1} / {2,3} in raster order
__device__ __forceinline__ uint32_t cluster_pixel_selector(const uint64_t* __restrict__ enc_blocks, const uint32_t* __restrict__ members, uint32_t j) {
    const uint32_t tv = members[j >> 3], k = j & 7u;
    const uint32_t lo32 = (uint32_t)bswap64(enc_blocks[tv >> 1]);
    return selector_from_bits(lo32, k & 3u, (tv & 1u) * 2u + (k >> 2));
}

// FORCED = the etc1_optimizer with m_pForce_selectors (etc.cpp:1188-1193): every texel is scored against the colour its current
// selector picks instead of the nearest one; the previous endpoints are never kept here, instead the cluster's CURRENT error
// (each texel against its own block's current colours) is returned in cur_err_out for the caller's "only if better" test.
template <bool PERCEPTUAL, int QUALITY, bool FORCED>
__global__ __launch_bounds__(CB_THREADS) void k_generate_endpoint_codebook(
    const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
    const uint32_t* __restrict__ indices, uint32_t step, uint8_t* __restrict__ params, uint64_t* __restrict__ err_out, uint8_t* __restrict__ valid,
    const uint64_t* __restrict__ enc_blocks, uint64_t* __restrict__ cur_err_out) {
    __shared__ uint64_t s_part[CB_WAVES][8];
    __shared__ uint64_t s_tot[8];
    __shared__ int s_mm[CB_WAVES][6];
    __shared__ uint32_t s_bloom[32];
    __shared__ float s_avg[3];
    __shared__ int s_spread;
    __shared__ int s_active;
    __shared__ uint32_t s_px[CB_STAGE];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ci = order[blockIdx.x];
    const uint32_t first = offsets[ci];
    const uint32_t n = (offsets[ci + 1] - first) * 8u; // pixels
    const uint32_t* members = indices + first;
    auto texel = [&](uint32_t j) -> uint32_t { return j < CB_STAGE ? s_px[j] : cluster_pixel(pixel_words, members, j); };   // valid after the init pass

    if (tid < 32) s_bloom[tid] = 0;

    // ---- init: channel sums, min/max
    {
        uint64_t sr = 0, sg = 0, sb = 0;
        int mn_r = 255, mn_g = 255, mn_b = 255, mx_r = 0, mx_g = 0, mx_b = 0;
        for (uint32_t j = tid; j < n; j += CB_THREADS) {
            const uint32_t w = cluster_pixel(pixel_words, members, j);
            if (j < CB_STAGE) s_px[j] = w;
            const int r = w & 255, g = (w >> 8) & 255, b = (w >> 16) & 255;
            sr += r; sg += g; sb += b;
            mn_r = min(mn_r, r); mn_g = min(mn_g, g); mn_b = min(mn_b, b);
            mx_r = max(mx_r, r); mx_g = max(mx_g, g); mx_b = max(mx_b, b);
        }
        sr = wave_allsum_u64(sr); sg = wave_allsum_u64(sg); sb = wave_allsum_u64(sb);
        mn_r = wave_min_i32(mn_r); mn_g = wave_min_i32(mn_g); mn_b = wave_min_i32(mn_b);
        mx_r = wave_max_i32(mx_r); mx_g = wave_max_i32(mx_g); mx_b = wave_max_i32(mx_b);
        if (lane == 0) {
            s_part[wave][0] = sr; s_part[wave][1] = sg; s_part[wave][2] = sb;
            s_mm[wave][0] = mn_r; s_mm[wave][1] = mn_g; s_mm[wave][2] = mn_b;
            s_mm[wave][3] = mx_r; s_mm[wave][4] = mx_g; s_mm[wave][5] = mx_b;
        }
    }
    __syncthreads();
    if (tid < 3) {
        uint64_t s = 0;
        for (int w = 0; w < CB_WAVES; w++) s += s_part[w][tid];
        float fs;
        if (s <= (1ull << 24)) {
            fs = (float)s; // every partial sum of the reference's running float sum is an exactly representable integer
        } else {
            fs = 0.0f;     // replay the float accumulation in pixel order (etc.cpp:1034-1041)
            for (uint32_t j = 0; j < n; j++) fs += (float)((texel(j) >> (8 * tid)) & 255u);
        }
        s_avg[tid] = fs / (float)n;
    }
    if (tid == 0) {
        int mn[3] = {255, 255, 255}, mx[3] = {0, 0, 0};
        for (int w = 0; w < CB_WAVES; w++)
            for (int c = 0; c < 3; c++) { mn[c] = min(mn[c], s_mm[w][c]); mx[c] = max(mx[c], s_mm[w][3 + c]); }
        s_spread = max(max(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    }
    __syncthreads();
    const float avg_r = s_avg[0], avg_g = s_avg[1], avg_b = s_avg[2];
    const uint32_t enable_mask = (QUALITY > BU_Q_MEDIUM) ? 0xFFu : (uint32_t)c_inten_enable_by_spread[s_spread];

    uint64_t best_err = ~0ull;
    int best_r = 0, best_g = 0, best_b = 0, best_inten = 0;
    bool best_valid = false;

    const int perms = (int)perms_for_quality(QUALITY);
    for (int i = -1; i < perms; i++) {
        int tr = 0, tg = 0, tb = 0;
        bool active = true;
        if (i < 0) {
            tr = avg_to_color5(avg_r); tg = avg_to_color5(avg_g); tb = avg_to_color5(avg_b);
        } else {
            active = cluster_fit_trial(c_cluster_fit_order[i], best_r, best_g, best_b, best_inten, avg_r, avg_g, avg_b, tr, tg, tb);
        }
        // all threads hold identical state, so `active` is workgroup-uniform; thread 0 owns the Bloom filter
        if (tid == 0) s_active = active ? (bloom_test_and_set(s_bloom, tr, tg, tb) ? 1 : 0) : 0;
        __syncthreads();
        active = s_active != 0;
        if (active) {
            cvec bc[8][4];
#pragma unroll
            for (int t = 0; t < 8; t++) block_cvecs<PERCEPTUAL>(bc[t], scale5(tr), scale5(tg), scale5(tb), t);
            uint64_t tot[8];
#pragma unroll
            for (int t = 0; t < 8; t++) tot[t] = 0;
            uint32_t plain_mask = 0;   // workgroup-uniform
#pragma unroll
            for (int t = 0; t < 8; t++) plain_mask |= base_unclamped(scale5(tr), scale5(tg), scale5(tb), t) ? (1u << t) : 0u;
            plain_mask &= enable_mask;
            const cvec base_cv = to_cvec<PERCEPTUAL>(scale5(tr), scale5(tg), scale5(tb));
            uint32_t clamp_bits = 0;   // bit 4 t + k: colour k of table t clamps a channel (workgroup-uniform)
            {
                const int base_mn = min(scale5(tr), min(scale5(tg), scale5(tb))), base_mx = max(scale5(tr), max(scale5(tg), scale5(tb)));
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    if (base_mn - k_inten_b[t] < 0) clamp_bits |= 1u << (t * 4);
                    if (base_mn - k_inten_a[t] < 0) clamp_bits |= 2u << (t * 4);
                    if (base_mx + k_inten_a[t] > 255) clamp_bits |= 4u << (t * 4);
                    if (base_mx + k_inten_b[t] > 255) clamp_bits |= 8u << (t * 4);
                }
            }
            for (uint32_t j = tid; j < n; j += CB_THREADS) {
                const cvec p = pixel_cvec<PERCEPTUAL>(texel(j));
                if (FORCED) {
                    const uint32_t sel = cluster_pixel_selector(enc_blocks, members, j);
#pragma unroll
                    for (int t = 0; t < 8; t++) {
                        const cvec c = select_cvec(bc[t], sel);
                        tot[t] += cdist<PERCEPTUAL>(p, c);
                    }
                } else if (PERCEPTUAL) {
                    // colours that need no clamping share the pixel's chroma term (etc1s_device.h, base_unclamped / mixed_min): a table none of whose colours clamp costs
                    // two squares, in the others only the clamped colours take the full distance (which ones: workgroup-uniform, scalar branches)
                    const uint32_t ch = chroma_term(p.y - base_cv.y, p.z - base_cv.z);
                    const int dx0 = p.x - base_cv.x;
#pragma unroll
                    for (int t = 0; t < 8; t++) {
                        if (!((enable_mask >> t) & 1u)) continue;
                        if ((plain_mask >> t) & 1u) {
                            tot[t] += min_luma_term(dx0, k_inten_a[t] * 64, k_inten_b[t] * 64) + ch;
                        } else {
                            mixed_min m = { ~0u, ~0u };
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int d = k == 0 ? -k_inten_b[t] : k == 1 ? -k_inten_a[t] : k == 2 ? k_inten_a[t] : k_inten_b[t];
                                if ((clamp_bits >> (t * 4 + k)) & 1u) {
                                    m.full = min(m.full, cdist<true>(p, bc[t][k]));
                                } else {
                                    const int e = dx0 - 64 * d;
                                    m.luma_sq = min(m.luma_sq, (uint32_t)__mul24(e, e));
                                }
                            }
                            tot[t] += mixed_min_total(m, ch);
                        }
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 8; t++)
                        if ((enable_mask >> t) & 1u) tot[t] += min_err4<PERCEPTUAL>(p, bc[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const uint64_t s = wave_allsum_u64(tot[t]);
                if (lane == 0) s_part[wave][t] = s;
            }
            __syncthreads();
            if (tid < 8) {
                uint64_t s = 0;
                for (int w = 0; w < CB_WAVES; w++) s += s_part[w][tid];
                s_tot[tid] = s;
            }
            __syncthreads();
            uint64_t trial_err = (uint64_t)INT64_MAX; // etc.cpp:1131
            int trial_inten = 0;
            bool trial_valid = false;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                if (!((enable_mask >> t) & 1u)) continue;
                const uint64_t s = s_tot[t];
                if (s < trial_err) { trial_err = s; trial_inten = t; trial_valid = true; }
            }
            if (trial_err < best_err) {
                best_err = trial_err; best_inten = trial_inten; best_valid = trial_valid;
                best_r = tr; best_g = tg; best_b = tb;
            }
        }
        __syncthreads(); // s_active / s_part / s_tot are reused by the next trial
        if (best_err == 0 || !best_valid) break; // etc.cpp:955-956, 993-994
    }

    if (FORCED) {
        // current error of the cluster's texels under their own blocks' present colours (frontend.cpp:2773)
        uint64_t tot = 0;
        for (uint32_t j = tid; j < n; j += CB_THREADS) {
            const uint32_t tv = members[j >> 3];
            uint32_t r5, g5, b5, inten;
            unpack_etc1s_header(enc_blocks[tv >> 1], r5, g5, b5, inten);
            cvec bc[4];
            block_cvecs<PERCEPTUAL>(bc, scale5((int)r5), scale5((int)g5), scale5((int)b5), (int)inten);
            const uint32_t sel = cluster_pixel_selector(enc_blocks, members, j);
            const cvec c = select_cvec(bc, (uint32_t)sel);
            tot += cdist<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(texel(j)), c);
        }
        tot = wave_allsum_u64(tot);
        __syncthreads();
        if (lane == 0) s_part[wave][0] = tot;
        __syncthreads();
        if (tid == 0) {
            uint64_t cur = 0;
            for (int w = 0; w < CB_WAVES; w++) cur += s_part[w][0];
            cur_err_out[ci] = cur;
            params[ci * 4 + 0] = (uint8_t)best_r; params[ci * 4 + 1] = (uint8_t)best_g; params[ci * 4 + 2] = (uint8_t)best_b; params[ci * 4 + 3] = (uint8_t)best_inten;
            err_out[ci] = best_err;
            valid[ci] = best_valid ? 1 : 0;
        }
        return;
    }
    // ---- keep the previous endpoints unless the error strictly drops (frontend.cpp:1554-1605)
    bool use_new = true;
    if (step != 0 && valid[ci]) {
        const int pr = params[ci * 4 + 0], pg = params[ci * 4 + 1], pb = params[ci * 4 + 2], pi = params[ci * 4 + 3];
        cvec bc[4];
        block_cvecs<PERCEPTUAL>(bc, scale5(pr), scale5(pg), scale5(pb), pi);
        uint64_t tot = 0;
        for (uint32_t j = tid; j < n; j += CB_THREADS) tot += min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(texel(j)), bc);
        tot = wave_allsum_u64(tot);
        if (lane == 0) s_part[wave][0] = tot;
        __syncthreads();
        uint64_t prev = 0;
        for (int w = 0; w < CB_WAVES; w++) prev += s_part[w][0];
        use_new = prev > best_err;
    }
    if (tid == 0 && use_new) {
        params[ci * 4 + 0] = (uint8_t)best_r; params[ci * 4 + 1] = (uint8_t)best_g; params[ci * 4 + 2] = (uint8_t)best_b; params[ci * 4 + 3] = (uint8_t)best_inten;
        err_out[ci] = best_err;
        valid[ci] = 1;
    }
}

#include "etc1s_codebook_wide.inc"

hipError_t launch_generate_endpoint_codebook(hipStream_t st, const void* d_pixel_blocks, uint32_t n_clusters, const uint32_t* d_order,
                                             const uint32_t* d_offsets, const uint32_t* d_indices, int quality, bool perceptual, uint32_t step,
                                             uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid) {
    if (!n_clusters) return hipSuccess;
    // the etc1_optimizer never runs at "fast" quality for clusters (frontend.cpp:1530-1533)
    if (quality < BU_Q_MEDIUM) quality = BU_Q_MEDIUM;
    with_bool(perceptual, [&](auto p) { with_quality<BU_Q_MEDIUM>(quality, [&](auto q) {
        hipLaunchKernelGGL((k_generate_endpoint_codebook<decltype(p)::value, decltype(q)::value, false>), dim3(n_clusters), dim3(CB_THREADS), 0, st,
                           static_cast<const uint32_t*>(d_pixel_blocks), d_order, d_offsets, d_indices, step, d_params, d_err, d_valid, (const uint64_t*)nullptr, (uint64_t*)nullptr);
    }); });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

// refine_block_endpoints_given_selectors (frontend.cpp:2718-2976) / reoptimize_remapped_endpoints (:2996-3104): cluster fit with the selectors held fixed
hipError_t launch_refit_endpoints_given_selectors(hipStream_t st, const void* d_pixel_blocks, const void* d_enc_blocks, uint32_t n_clusters, const uint32_t* d_order,
                                                  const uint32_t* d_offsets, const uint32_t* d_indices, int quality, bool perceptual, uint8_t* d_params, uint64_t* d_err,
                                                  uint8_t* d_valid, uint64_t* d_cur_err) {
    if (!n_clusters) return hipSuccess;
    // uber for refine_block_endpoints_given_selectors and level 6; slow for reoptimize_remapped_endpoints below level 6 (frontend.cpp:3073-3076)
    with_bool(perceptual, [&](auto p) { with_quality<BU_Q_SLOW>(quality, [&](auto q) {
        hipLaunchKernelGGL((k_generate_endpoint_codebook<decltype(p)::value, decltype(q)::value, true>), dim3(n_clusters), dim3(CB_THREADS), 0, st,
                           static_cast<const uint32_t*>(d_pixel_blocks), d_order, d_offsets, d_indices, 0u, d_params, d_err, d_valid, static_cast<const uint64_t*>(d_enc_blocks), d_cur_err);
    }); });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace bu
