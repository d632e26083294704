// etc1s_block_fit_kernels.hip -- a6: the per-block etc1_optimizer of init_etc1_images (three kernels: the general one, the perceptual one with the lanes
// turned to pixels, and the level-0 variant). Design rules of the ETC1S kernels: etc1s_kernels.h.
#include "etc1s_fit_common.h"
#include "launch_dispatch.h"

namespace bu {

hipError_t upload_block_fit_tables() { return upload_fit_tables(); }

// -------------------------------------------------------------------------------------------------------------------
// a6: init_etc1_images -- per 4x4 block etc1_optimizer (frontend.cpp:765-818; etc.cpp:776-1278)
//
// Mapping: 8 lanes per block (lane = intensity table), 8 blocks per wave, 32 blocks per 256-thread workgroup.
// Every lane keeps the block's 16 pixels in registers; a trial base colour costs each lane one pass over 16 pixels x 4
// selectors for ITS table; the best table is an 8-lane min-reduction on key (error << 3 | table), which reproduces the
// reference's ascending-table strict-< scan. Trial colours depend on the running best solution, so trials are serial.
// -------------------------------------------------------------------------------------------------------------------

template <bool PERCEPTUAL, int QUALITY>
__global__ __launch_bounds__(256) void k_encode_etc1s_blocks(const uint4* __restrict__ pixel_blocks, uint32_t n_blocks, uint2* __restrict__ out_blocks) {
    __shared__ uint32_t s_bloom[32][32];

    const uint32_t tid = threadIdx.x;
    const uint32_t table = tid & 7u;
    const uint32_t slot = tid >> 3;
    const uint32_t group_shift = tid & 56u; // where this block's 8 lanes sit in a wave-wide ballot
    const uint32_t block_raw = blockIdx.x * 32u + slot;
    const bool in_range = block_raw < n_blocks;
    const uint32_t block = in_range ? block_raw : (n_blocks - 1);

    // clear this block's Bloom filter (8 lanes x 4 dwords)
#pragma unroll
    for (int i = 0; i < 4; i++) s_bloom[slot][table * 4 + i] = 0;

    // 64-byte tile: four 16-byte loads, identical for the 8 lanes of a block (served by one cache line)
    uint32_t px[16];
    {
        const uint4* src = pixel_blocks + (size_t)block * 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = src[i];
            px[i * 4 + 0] = v.x; px[i * 4 + 1] = v.y; px[i * 4 + 2] = v.z; px[i * 4 + 3] = v.w;
        }
    }

    // etc1_optimizer::init (etc.cpp:998-1070)
    cvec pc[16];
    float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f;
    int mn_r = 255, mn_g = 255, mn_b = 255, mx_r = 0, mx_g = 0, mx_b = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = px[i] & 255, g = (px[i] >> 8) & 255, b = (px[i] >> 16) & 255;
        mn_r = min(mn_r, r); mn_g = min(mn_g, g); mn_b = min(mn_b, b);
        mx_r = max(mx_r, r); mx_g = max(mx_g, g); mx_b = max(mx_b, b);
        sum_r += (float)r; sum_g += (float)g; sum_b += (float)b;
        pc[i] = to_cvec<PERCEPTUAL>(r, g, b);
    }
    const float avg_r = sum_r / 16.0f, avg_g = sum_g / 16.0f, avg_b = sum_b / 16.0f;
    const int spread = max(max(mx_r - mn_r, mx_g - mn_g), mx_b - mn_b);
    const bool table_enabled = (QUALITY > BU_Q_MEDIUM) ? true : (((uint32_t)c_inten_enable_by_spread[spread] >> table) & 1u) != 0; // etc.cpp:1135-1140

    uint32_t best_err = 0xFFFFFFFFu; // every real total is < 2^28
    int best_r = 0, best_g = 0, best_b = 0, best_inten = 0;

    __syncthreads(); // filters cleared

    // Trials: every block at its own pace, eight trial colours per generation (see k_encode_etc1s_blocks_by_pixel below, which explains the scheme)
    const int perms = (int)perms_for_quality(QUALITY);
    int batch_base = 0, mine_r = 0, mine_g = 0, mine_b = 0;
    bool mine_ok = false, batch_fresh = false;
    uint32_t mine_h0 = 0, mine_h1 = 0;
    int next = -1;                    // the first trial index this block has not dealt with; -1 = the average colour (etc.cpp:1047-1049)
    bool done = false;

    for (;;) {
        int pick = -1;                // lane of the block's batch whose trial it evaluates now
        if (next < 0) {
            pick = 0; next = 0;
            mine_r = avg_to_color5(avg_r); mine_g = avg_to_color5(avg_g); mine_b = avg_to_color5(avg_b);
            const uint32_t kh = hash_hsieh3((uint32_t)mine_r, (uint32_t)mine_g, (uint32_t)mine_b);
            mine_h0 = kh & 1023u; mine_h1 = (kh >> 10) & 1023u;
        } else {
            bool searching = !done;
            while (__any(searching)) {
                if (searching && !batch_fresh) {
                    batch_base = next; batch_fresh = true;
                    const int idx = batch_base + (int)table;
                    mine_ok = idx < perms &&
                              cluster_fit_trial(c_cluster_fit_order[min(idx, perms - 1)], best_r, best_g, best_b, best_inten, avg_r, avg_g, avg_b, mine_r, mine_g, mine_b);
                    const uint32_t kh = hash_hsieh3((uint32_t)mine_r, (uint32_t)mine_g, (uint32_t)mine_b);
                    mine_h0 = kh & 1023u; mine_h1 = (kh >> 10) & 1023u;
                }
                bool fresh_colour = false;
                if (searching && mine_ok && batch_base + (int)table >= next) {
                    const uint32_t w0 = s_bloom[slot][mine_h0 >> 5], w1 = s_bloom[slot][mine_h1 >> 5];
                    fresh_colour = !(((w0 >> (mine_h0 & 31u)) & 1u) && ((w1 >> (mine_h1 & 31u)) & 1u));
                }
                const uint32_t m8 = (uint32_t)(__ballot(fresh_colour) >> group_shift) & 0xFFu;
                if (searching) {
                    if (m8) {
                        pick = __ffs((int)m8) - 1;
                        next = batch_base + pick + 1;
                        searching = false;
                    } else {
                        next = batch_base + 8; batch_fresh = false;
                        if (next >= perms) { done = true; searching = false; }
                    }
                }
            }
        }
        if (__all(done)) break;
        const bool active = pick >= 0;
        const int src_lane = active ? pick : 0;
        const int tr = __shfl(mine_r, src_lane, 8), tg = __shfl(mine_g, src_lane, 8), tb = __shfl(mine_b, src_lane, 8);
        if (active) {
            // check_for_redundant_solution's insertion (etc.cpp:1072-1089): the 8 lanes write the same values
            const uint32_t h0 = (uint32_t)__shfl((int)mine_h0, src_lane, 8), h1 = (uint32_t)__shfl((int)mine_h1, src_lane, 8);
            atomicOr(&s_bloom[slot][h0 >> 5], 1u << (h0 & 31u));
            atomicOr(&s_bloom[slot][h1 >> 5], 1u << (h1 & 31u));
        }
        {
            // evaluate_solution_slow (etc.cpp:1104-1278): this lane's table only
            uint32_t total = 0x0FFFFFFFu;
            if (active && table_enabled) {
                cvec bc[4];
                block_cvecs<PERCEPTUAL>(bc, scale5(tr), scale5(tg), scale5(tb), (int)table);
                total = 0;
#pragma unroll
                for (int p = 0; p < 16; p++) total += min_err4<PERCEPTUAL>(pc[p], bc);
            }
            uint32_t key = (total << 3) | table;
            key = min(key, (uint32_t)__shfl_xor((int)key, 1, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 2, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 4, 8));
            const uint32_t trial_err = key >> 3;
            if (active && trial_err < best_err) {
                best_err = trial_err; best_inten = (int)(key & 7u);
                best_r = tr; best_g = tg; best_b = tb;
                batch_fresh = false;              // the trials after this one start from the new best solution
            }
        }
        if (best_err == 0 || next >= perms) done = true; // etc.cpp:955-956, 993-994
    }

    // Selectors of the winning (colour, table): each of the 8 lanes classifies 2 pixels, first-min over s (etc.cpp:1188-1219).
    cvec bc[4];
    block_cvecs<PERCEPTUAL>(bc, scale5(best_r), scale5(best_g), scale5(best_b), best_inten);
    uint32_t bits = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        if ((uint32_t)(p >> 1) == table) {
            const uint32_t s = best_sel4<PERCEPTUAL>(pc[p], bc);
            bits |= selector_bits((uint32_t)(p & 3), (uint32_t)(p >> 2), s);
        }
    }
    bits |= (uint32_t)__shfl_xor((int)bits, 1, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 2, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 4, 8);
    if (table == 0 && in_range) {
        const uint64_t v = etc1s_header_bits((uint32_t)best_r, (uint32_t)best_g, (uint32_t)best_b, (uint32_t)best_inten) | bits;
        const uint64_t m = bswap64(v);
        out_blocks[block] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
}

// The same for the perceptual metric with the lanes turned by ninety degrees: the 8 lanes of a block each own TWO PIXELS and
// walk all the enabled tables. A trial colour whose table needs no clamping then costs a lane one chroma term per pixel
// (shared by all such tables) and one luma minimum per pixel and table (etc1s_device.h, base_unclamped) instead of four full
// distances; clamped tables take the four-distance form as before. The per-table totals of the 8 lanes meet in a three-step
// exchange that leaves lane l with the complete total of one table, and from there on the reduction is the one above.
//
// Trials. Most of a block's 1 + perms trial colours are ones it has seen (check_for_redundant_solution): 4.2 of 17 are
// evaluated per block of the bench image, but WHICH ones differs from block to block, and a wave that steps its 8 blocks
// through the trial indices together evaluates the union (10.4 of 17). Here every block moves at its own pace: its 8 lanes
// make the next EIGHT trial colours from the current best solution at once (lane l: trial next + l), the first of them
// the filter does not know is evaluated, and only an evaluation that improves the best solution -- the one thing later
// trial colours depend on -- makes the lanes generate again. A trial the filter knew when it was looked at stays known
// (the filter only grows), a trial is entered into the filter when it is evaluated and not before: the sequence of
// (colour, filter state) pairs is the reference's. A wave evaluates max-over-blocks trials (5.2) instead of the union.
template <int QUALITY>
__global__ __launch_bounds__(256) void k_encode_etc1s_blocks_by_pixel(const uint4* __restrict__ pixel_blocks, uint32_t n_blocks, uint2* __restrict__ out_blocks) {
    __shared__ uint32_t s_bloom[32][32];

    const uint32_t tid = threadIdx.x;
    const uint32_t sub = tid & 7u;        // pixels 2 sub, 2 sub + 1
    const uint32_t slot = tid >> 3;
    const uint32_t group_shift = tid & 56u; // where this block's 8 lanes sit in a wave-wide ballot
    const uint32_t block_raw = blockIdx.x * 32u + slot;
    const bool in_range = block_raw < n_blocks;
    const uint32_t block = in_range ? block_raw : (n_blocks - 1);
#pragma unroll
    for (int i = 0; i < 4; i++) s_bloom[slot][sub * 4 + i] = 0;

    // etc1_optimizer::init (etc.cpp:998-1070): every lane over all 16 pixels (the float sums must run in pixel order)
    float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f;
    int mn_r = 255, mn_g = 255, mn_b = 255, mx_r = 0, mx_g = 0, mx_b = 0;
    {
        const uint4* src = pixel_blocks + (size_t)block * 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = src[i];
            const uint32_t w4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int r = w4[k] & 255, g = (w4[k] >> 8) & 255, b = (w4[k] >> 16) & 255;
                mn_r = min(mn_r, r); mn_g = min(mn_g, g); mn_b = min(mn_b, b);
                mx_r = max(mx_r, r); mx_g = max(mx_g, g); mx_b = max(mx_b, b);
                sum_r += (float)r; sum_g += (float)g; sum_b += (float)b;
            }
        }
    }
    const uint2 mine = reinterpret_cast<const uint2*>(pixel_blocks + (size_t)block * 4)[sub];
    const cvec pc0 = pixel_cvec<true>(mine.x), pc1 = pixel_cvec<true>(mine.y);
    const float avg_r = sum_r / 16.0f, avg_g = sum_g / 16.0f, avg_b = sum_b / 16.0f;
    const int spread = max(max(mx_r - mn_r, mx_g - mn_g), mx_b - mn_b);
    const uint32_t enable_mask = (QUALITY > BU_Q_MEDIUM) ? 0xFFu : (uint32_t)c_inten_enable_by_spread[spread]; // etc.cpp:1135-1140
    // the table this lane ends up holding the total of (see the exchange below)
    const uint32_t my_table = ((sub & 1u) << 2) | (sub & 2u) | ((sub >> 2) & 1u);

    uint32_t best_err = 0xFFFFFFFFu; // every real total is < 2^28
    int best_r = 0, best_g = 0, best_b = 0, best_inten = 0;

    __syncthreads(); // filters cleared

    const int perms = (int)perms_for_quality(QUALITY);
    // what this lane holds of the block's current batch of trials: trial batch_base + sub, made from the best solution as it was then
    int batch_base = 0, mine_r = 0, mine_g = 0, mine_b = 0;
    bool mine_ok = false, batch_fresh = false;
    uint32_t mine_h0 = 0, mine_h1 = 0;
    int next = -1;                    // the first trial index this block has not dealt with; -1 = the average colour (etc.cpp:1047-1049)
    bool done = false;

    for (;;) {
        // ---- which trial does each block evaluate next? (blocks that find none are done)
        int pick = -1;                // lane of the block's batch whose trial it is
        if (next < 0) {
            pick = 0; next = 0;
            mine_r = avg_to_color5(avg_r); mine_g = avg_to_color5(avg_g); mine_b = avg_to_color5(avg_b);
            const uint32_t kh = hash_hsieh3((uint32_t)mine_r, (uint32_t)mine_g, (uint32_t)mine_b);
            mine_h0 = kh & 1023u; mine_h1 = (kh >> 10) & 1023u;
        } else {
            bool searching = !done;
            while (__any(searching)) {
                if (searching && !batch_fresh) {
                    batch_base = next; batch_fresh = true;
                    const int idx = batch_base + (int)sub;
                    mine_ok = idx < perms &&
                              cluster_fit_trial(c_cluster_fit_order[min(idx, perms - 1)], best_r, best_g, best_b, best_inten, avg_r, avg_g, avg_b, mine_r, mine_g, mine_b);
                    const uint32_t kh = hash_hsieh3((uint32_t)mine_r, (uint32_t)mine_g, (uint32_t)mine_b);
                    mine_h0 = kh & 1023u; mine_h1 = (kh >> 10) & 1023u;
                }
                bool fresh_colour = false;
                if (searching && mine_ok && batch_base + (int)sub >= next) {
                    const uint32_t w0 = s_bloom[slot][mine_h0 >> 5], w1 = s_bloom[slot][mine_h1 >> 5];
                    fresh_colour = !(((w0 >> (mine_h0 & 31u)) & 1u) && ((w1 >> (mine_h1 & 31u)) & 1u));
                }
                const uint32_t m8 = (uint32_t)(__ballot(fresh_colour) >> group_shift) & 0xFFu;
                if (searching) {
                    if (m8) {
                        pick = __ffs((int)m8) - 1;
                        next = batch_base + pick + 1;
                        searching = false;
                    } else {
                        next = batch_base + 8; batch_fresh = false;
                        if (next >= perms) { done = true; searching = false; }
                    }
                }
            }
        }
        if (__all(done)) break;
        const bool active = pick >= 0;
        const int src_lane = active ? pick : 0;
        const int tr = __shfl(mine_r, src_lane, 8), tg = __shfl(mine_g, src_lane, 8), tb = __shfl(mine_b, src_lane, 8);
        if (active) {
            // check_for_redundant_solution's insertion (etc.cpp:1072-1089): the 8 lanes write the same values
            const uint32_t h0 = (uint32_t)__shfl((int)mine_h0, src_lane, 8), h1 = (uint32_t)__shfl((int)mine_h1, src_lane, 8);
            atomicOr(&s_bloom[slot][h0 >> 5], 1u << (h0 & 31u));
            atomicOr(&s_bloom[slot][h1 >> 5], 1u << (h1 & 31u));
        }
        // evaluate_solution_slow (etc.cpp:1104-1278): this lane's two pixels against every enabled table
        const int br = scale5(tr), bg = scale5(tg), bb = scale5(tb);
        const cvec base_cv = to_cvec<true>(br, bg, bb);
        const uint32_t todo = active ? enable_mask : 0u;
        const uint32_t ch0 = chroma_term(pc0.y - base_cv.y, pc0.z - base_cv.z), ch1 = chroma_term(pc1.y - base_cv.y, pc1.z - base_cv.z);
        const int dx0 = pc0.x - base_cv.x, dx1 = pc1.x - base_cv.x;
        const int base_mn = min(br, min(bg, bb)), base_mx = max(br, max(bg, bb));
        uint32_t tot[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            tot[t] = 0;
            if (!((todo >> t) & 1u)) continue;
            if (base_unclamped(br, bg, bb, t)) {
                tot[t] = min_luma_term(dx0, k_inten_a[t] * 64, k_inten_b[t] * 64) + ch0 + min_luma_term(dx1, k_inten_a[t] * 64, k_inten_b[t] * 64) + ch1;
            } else {
                // some of the four colours clamp: the others keep the base colour's chroma (one square each), the clamped ones take the full distance
                mixed_min m0 = { ~0u, ~0u }, m1 = { ~0u, ~0u };
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int d = k == 0 ? -k_inten_b[t] : k == 1 ? -k_inten_a[t] : k == 2 ? k_inten_a[t] : k_inten_b[t];
                    const bool clamps = d < 0 ? base_mn + d < 0 : base_mx + d > 255;
                    const int e0 = dx0 - 64 * d, e1 = dx1 - 64 * d;
                    m0.luma_sq = min(m0.luma_sq, clamps ? ~0u : (uint32_t)__mul24(e0, e0));
                    m1.luma_sq = min(m1.luma_sq, clamps ? ~0u : (uint32_t)__mul24(e1, e1));
                    if (clamps) {
                        const cvec c = to_cvec<true>(clamp255(br + d), clamp255(bg + d), clamp255(bb + d));
                        m0.full = min(m0.full, cdist<true>(pc0, c));
                        m1.full = min(m1.full, cdist<true>(pc1, c));
                    }
                }
                tot[t] = mixed_min_total(m0, ch0) + mixed_min_total(m1, ch1);
            }
        }
        // exchange: after the step with partner distance d the lane keeps the half of its tables selected by its bit d
        uint32_t k4[4], k2[2], k1;
        {
            const bool up = (sub & 1u) != 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t give = up ? tot[k] : tot[4 + k];
                k4[k] = (up ? tot[4 + k] : tot[k]) + (uint32_t)__shfl_xor((int)give, 1, 8);
            }
        }
        {
            const bool up = (sub & 2u) != 0;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const uint32_t give = up ? k4[k] : k4[2 + k];
                k2[k] = (up ? k4[2 + k] : k4[k]) + (uint32_t)__shfl_xor((int)give, 2, 8);
            }
        }
        {
            const bool up = (sub & 4u) != 0;
            const uint32_t give = up ? k2[0] : k2[1];
            k1 = (up ? k2[1] : k2[0]) + (uint32_t)__shfl_xor((int)give, 4, 8);
        }
        {
            const uint32_t total = ((enable_mask >> my_table) & 1u) ? k1 : 0x0FFFFFFFu;
            uint32_t key = (total << 3) | my_table;
            key = min(key, (uint32_t)__shfl_xor((int)key, 1, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 2, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 4, 8));
            const uint32_t trial_err = key >> 3;
            if (active && trial_err < best_err) {
                best_err = trial_err; best_inten = (int)(key & 7u);
                best_r = tr; best_g = tg; best_b = tb;
                batch_fresh = false;              // the trials after this one start from the new best solution
            }
        }
        if (best_err == 0 || next >= perms) done = true; // etc.cpp:955-956, 993-994
    }

    // Selectors of the winning (colour, table): first-min over s (etc.cpp:1188-1219), two pixels per lane
    cvec bc[4];
    block_cvecs<true>(bc, scale5(best_r), scale5(best_g), scale5(best_b), best_inten);
    const uint32_t p0 = sub * 2u, p1 = p0 + 1u;
    uint32_t bits = selector_bits(p0 & 3u, p0 >> 2, best_sel4<true>(pc0, bc)) | selector_bits(p1 & 3u, p1 >> 2, best_sel4<true>(pc1, bc));
    bits |= (uint32_t)__shfl_xor((int)bits, 1, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 2, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 4, 8);
    if (sub == 0 && in_range) {
        const uint64_t v = etc1s_header_bits((uint32_t)best_r, (uint32_t)best_g, (uint32_t)best_b, (uint32_t)best_inten) | bits;
        const uint64_t m = bswap64(v);
        out_blocks[block] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
}

// Level-0 variant: evaluate_solution_fast (etc.cpp:1280-1506). Linear metric is forced (:1313); a pixel's selector is the
// number of block-colour luma midpoints at or below twice its luma; tables are scanned 7..0 with strict <, so on equal error
// the HIGHEST table wins -> reduction key uses (7 - table).
template <bool PERCEPTUAL_UNUSED>
__global__ __launch_bounds__(256) void k_encode_etc1s_blocks_fast(const uint4* __restrict__ pixel_blocks, uint32_t n_blocks, uint2* __restrict__ out_blocks) {
    __shared__ uint32_t s_bloom[32][32];
    const uint32_t tid = threadIdx.x;
    const uint32_t table = tid & 7u;
    const uint32_t slot = tid >> 3;
    const uint32_t block_raw = blockIdx.x * 32u + slot;
    const bool in_range = block_raw < n_blocks;
    const uint32_t block = in_range ? block_raw : (n_blocks - 1);
#pragma unroll
    for (int i = 0; i < 4; i++) s_bloom[slot][table * 4 + i] = 0;

    uint32_t px[16];
    {
        const uint4* src = pixel_blocks + (size_t)block * 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = src[i];
            px[i * 4 + 0] = v.x; px[i * 4 + 1] = v.y; px[i * 4 + 2] = v.z; px[i * 4 + 3] = v.w;
        }
    }
    cvec pc[16];
    uint32_t luma2[16];
    float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = px[i] & 255, g = (px[i] >> 8) & 255, b = (px[i] >> 16) & 255;
        sum_r += (float)r; sum_g += (float)g; sum_b += (float)b;
        pc[i] = to_cvec<false>(r, g, b);
        luma2[i] = (uint32_t)(r + g + b) * 2u;
    }
    const float avg_r = sum_r / 16.0f, avg_g = sum_g / 16.0f, avg_b = sum_b / 16.0f;

    uint32_t best_err = 0xFFFFFFFFu;
    int best_r = 0, best_g = 0, best_b = 0, best_inten = 0;
    bool done = false;
    __syncthreads();

    for (int i = -1; i < 4; i++) {
        if (__all(done)) break;
        bool active = !done;
        int tr = 0, tg = 0, tb = 0;
        if (i < 0) {
            tr = avg_to_color5(avg_r); tg = avg_to_color5(avg_g); tb = avg_to_color5(avg_b);
        } else if (active) {
            active = cluster_fit_trial(c_cluster_fit_order[i], best_r, best_g, best_b, best_inten, avg_r, avg_g, avg_b, tr, tg, tb);
        }
        if (active) active = bloom_test_and_set(&s_bloom[slot][0], tr, tg, tb);
        if (active) {
            cvec bc[4];
            block_cvecs<false>(bc, scale5(tr), scale5(tg), scale5(tb), (int)table);
            const uint32_t i0 = (uint32_t)(bc[0].x + bc[0].y + bc[0].z), i1 = (uint32_t)(bc[1].x + bc[1].y + bc[1].z);
            const uint32_t i2 = (uint32_t)(bc[2].x + bc[2].y + bc[2].z), i3 = (uint32_t)(bc[3].x + bc[3].y + bc[3].z);
            const uint32_t m0 = i0 + i1, m1 = i1 + i2, m2 = i2 + i3;
            uint32_t total = 0;
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t s = (uint32_t)(luma2[p] >= m0) + (uint32_t)(luma2[p] >= m1) + (uint32_t)(luma2[p] >= m2);
                // midpoints are non-decreasing, so the count equals the reference's walk (etc.cpp:1368-1376)
                const cvec c = select_cvec(bc, s);
                total += cdist<false>(pc[p], c);
            }
            uint32_t key = (total << 3) | (7u - table);
            key = min(key, (uint32_t)__shfl_xor((int)key, 1, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 2, 8));
            key = min(key, (uint32_t)__shfl_xor((int)key, 4, 8));
            const uint32_t trial_err = key >> 3;
            if (trial_err < best_err) {
                best_err = trial_err; best_inten = (int)(7u - (key & 7u));
                best_r = tr; best_g = tg; best_b = tb;
            }
        }
        if (best_err == 0) done = true;
    }

    cvec bc[4];
    block_cvecs<false>(bc, scale5(best_r), scale5(best_g), scale5(best_b), best_inten);
    const uint32_t i0 = (uint32_t)(bc[0].x + bc[0].y + bc[0].z), i1 = (uint32_t)(bc[1].x + bc[1].y + bc[1].z);
    const uint32_t i2 = (uint32_t)(bc[2].x + bc[2].y + bc[2].z), i3 = (uint32_t)(bc[3].x + bc[3].y + bc[3].z);
    const uint32_t m0 = i0 + i1, m1 = i1 + i2, m2 = i2 + i3;
    uint32_t bits = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        if ((uint32_t)(p >> 1) == table) {
            const uint32_t s = (uint32_t)(luma2[p] >= m0) + (uint32_t)(luma2[p] >= m1) + (uint32_t)(luma2[p] >= m2);
            bits |= selector_bits((uint32_t)(p & 3), (uint32_t)(p >> 2), s);
        }
    }
    bits |= (uint32_t)__shfl_xor((int)bits, 1, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 2, 8);
    bits |= (uint32_t)__shfl_xor((int)bits, 4, 8);
    if (table == 0 && in_range) {
        const uint64_t v = etc1s_header_bits((uint32_t)best_r, (uint32_t)best_g, (uint32_t)best_b, (uint32_t)best_inten) | bits;
        const uint64_t m = bswap64(v);
        out_blocks[block] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
}

// Level 0 forces the linear metric (etc.cpp:1313) and the perceptual fit has its own kernel, so k_encode_etc1s_blocks itself is only ever built for the linear metric.
hipError_t launch_encode_etc1s_blocks(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, int quality, bool perceptual, void* d_out) {
    if (!n_blocks) return hipSuccess;
    auto launch = [&](auto kernel) {   // (the three kernels have one signature)
        hipLaunchKernelGGL(kernel, dim3((n_blocks + 31) / 32), dim3(256), 0, st, static_cast<const uint4*>(d_pixel_blocks), n_blocks, static_cast<uint2*>(d_out));
    };
    if (quality == BU_Q_FAST) launch(k_encode_etc1s_blocks_fast<false>);
    else with_quality<BU_Q_MEDIUM>(quality, [&](auto q) {
        constexpr int Q = decltype(q)::value;
        if (perceptual) launch(k_encode_etc1s_blocks_by_pixel<Q>); else launch(k_encode_etc1s_blocks<false, Q>);
    });
    BU_LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace bu
