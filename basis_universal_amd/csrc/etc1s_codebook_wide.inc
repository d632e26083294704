// etc1s_codebook_wide.inc -- a9 (generate_endpoint_codebook, frontend.cpp:1482-1613) and the cluster fit with forced selectors (frontend.cpp:2718-2976, 2996-3104)
// for LARGE clusters. Included by etc1s_cluster_fit_kernels.hip behind k_generate_endpoint_codebook, whose helpers it uses.
//
// k_generate_endpoint_codebook gives a cluster ONE workgroup. That is right for the synthetic bench image (2,416 clusters of ~7,000 texels) and wrong for
// photographs: a sky, a flat wall or a constant alpha plane is one cluster of 10^5-10^7 texels, and its workgroup walks it 17 times (the trials depend on each
// other) while 255 CUs wait -- 14 ms of the Kodak mosaic's 35 ms step, 75 ms of the endpoint cube's 108, where the whole launch takes 1.07 ms on the bench image.
// Here a large cluster is cut into chunks of CBW_CHUNK texels and every pass over its texels is a launch over the chunks of ALL large clusters:
//
//   k_cbw_init   per chunk:   channel sums, min / max, and the error under the previous parameters (step > 0) or the current one (forced selectors) -> atomics
//   k_cbw_mean   per cluster: the float colour mean. The reference's mean is a RUNNING float sum in texel order (etc.cpp:1034-1041, SURVEY hazard H4): exact
//                             while it stays <= 2^24, order dependent beyond. cbw_ordered_sum evaluates it without its order, exactly (below)
//   k_cbw_step   per cluster: the serial part of the trial loop (etc.cpp:948-1000) on one thread: take the trial just evaluated, keep the best, make the next
//                             trial colour from it (cluster_fit_trial), ask the Bloom filter, honour the two early-outs
//   k_cbw_eval   per chunk:   one trial -- all 8 intensity-table totals of the chunk's texels -> u64 atomics. Integer sums: any order
//   k_cbw_final  per cluster: keep the previous endpoints unless the error strictly drops (frontend.cpp:1554-1605); results
//
// (init, mean, step, {eval, step} x (trials), final) are enqueued blind; a finished cluster's workgroups return at once. Results are bit-identical to the
// one-workgroup kernel (tests run both on the same clusters); the host sends a cluster here from bu_hip_tuning::codebook_wide_min texels up.

constexpr uint32_t CBW_CHUNK = 4096;      // texels per workgroup of the per-chunk kernels
constexpr uint32_t CBW_SUM_CHUNK = 256;   // texels per map of the ordered sum

struct cb_wide_state {
    uint32_t cluster, first, n_texels, n_sum_chunks;       // host-filled: cluster index, first member (sub-block) in `indices`, texels, ceil(n_texels / CBW_SUM_CHUNK)
    uint64_t sum_scratch_at;                               // host-filled: this cluster's region of the ordered sum's scratch (8-byte entries)
    unsigned long long sum[3];
    int mn[3], mx[3];                                      // host-filled 255 / 0
    float avg[3]; int spread; uint32_t enable_mask;
    int i, active, tr, tg, tb;                             // trial loop: index of the trial in flight (-1 .. perms - 1), whether its totals are being gathered, its colour
    unsigned long long tot[8];
    unsigned long long best_err; int best_r, best_g, best_b, best_inten, best_valid, done;
    unsigned long long prev_tot;                           // error under the previous parameters (step > 0) / under the blocks' current colours (forced selectors)
    uint32_t bloom[32];
};
struct cb_wide_chunk { uint32_t big, first_texel; };

// ---------------------------------------------------------------------------------------------------------------- the ordered float sum
// fs = 0; for every texel in list order: fs += (float)value, value an integer in 0..255 -- evaluated by a whole workgroup.
// The running sum is a non-decreasing integer-valued float. While it is <= 2^24 every add is exact. Beyond, inside the binade [2^e, 2^(e+1)) it is m * u with
// u = 2^(e-23) and 2^23 <= m < 2^24, and adding v = q u + r (0 <= r < u) gives m + q + {0 if r < u/2, 1 if r > u/2, (m + q) & 1 on a tie}: the increment depends on
// m only through its PARITY, so a run of addends is a pair (increment for an even start, increment for an odd start), and such pairs compose associatively.
// A phase: per chunk of 256 texels the pair for the current u; a prefix composition over the chunks gives every chunk its start value; the first chunk whose
// end value reaches 2^24 is where the binade changes -- that ONE chunk is added texel by texel with real float adds from its exact start value, and the next
// phase starts behind it in the binade its end value lies in. At most eight binade changes (255 * 2^24 texels < 2^32). Phase zero is the exact region: u = 1.
struct cbw_map { uint32_t d0, d1; };
__device__ __forceinline__ cbw_map cbw_compose(cbw_map f, cbw_map g) { return { f.d0 + ((f.d0 & 1u) ? g.d1 : g.d0), f.d1 + (((1u + f.d1) & 1u) ? g.d1 : g.d0) }; }   // f first, then g

template <int THREADS>
__device__ float cbw_ordered_sum(const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ members, uint32_t n, uint32_t n_chunks, int channel, cbw_map* maps /* n_chunks, global */) {
    __shared__ cbw_map s_scan[THREADS];
    __shared__ float s_vals[CBW_SUM_CHUNK];
    __shared__ float s_f;
    __shared__ uint32_t s_cross, s_m;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_chunks + THREADS - 1) / THREADS;            // chunks per thread, contiguous
    const uint32_t c0 = min(tid * per, n_chunks), c1 = min(c0 + per, n_chunks);
    auto value = [&](uint32_t j) -> uint32_t { return (cluster_pixel(pixel_words, members, j) >> (8 * channel)) & 255u; };
    if (tid == 0) { s_f = 0.0f; }
    uint32_t start = 0;   // first chunk not yet added
    __syncthreads();
    for (int phase = 0; phase < 12 && start < n_chunks; phase++) {
        const float f = s_f;
        const uint32_t bits = __float_as_uint(f);
        const int e = (int)((bits >> 23) & 255u) - 127;
        const bool exact_region = f < 16777216.0f;                      // every add exact while the sum stays <= 2^24
        const uint32_t k = exact_region ? 0u : (uint32_t)(e - 23);      // u = 2^k
        const uint32_t m0 = exact_region ? (uint32_t)f : ((bits & 0x7FFFFFu) | 0x800000u);
        const uint32_t limit = 16777216u;                               // exact region: the sum may REACH 2^24; a binade ends BEFORE m = 2^24
        // (1) per chunk: the pair of increments for an even / odd start
        for (uint32_t c = max(c0, start); c < c1; c++) {
            uint32_t d0 = 0, d1 = 0;
            const uint32_t j0 = c * CBW_SUM_CHUNK, j1 = min(j0 + CBW_SUM_CHUNK, n);
            if (k == 0) { for (uint32_t j = j0; j < j1; j++) d0 += value(j); d1 = d0; }
            else {
                const uint32_t half = 1u << (k - 1), rmask = (1u << k) - 1u;
                for (uint32_t j = j0; j < j1; j++) {
                    const uint32_t v = value(j), q = v >> k, r = v & rmask;
                    const uint32_t up = r > half ? 1u : 0u, tie = r == half ? 1u : 0u;
                    d0 += q + up + (tie & (d0 + q));            // start even: parity of m + q is that of d0 + q
                    d1 += q + up + (tie & (1u + d1 + q));       // start odd
                }
            }
            maps[c] = { d0, d1 };
        }
        // (2) every thread's chunks composed, then an inclusive scan of the threads' maps (Hillis-Steele: composition is associative, not commutative)
        cbw_map mine = { 0u, 0u };
        for (uint32_t c = max(c0, start); c < c1; c++) mine = cbw_compose(mine, maps[c]);
        s_scan[tid] = mine;
        __syncthreads();
        for (uint32_t o = 1; o < (uint32_t)THREADS; o <<= 1) {
            cbw_map left = { 0u, 0u };
            const bool have = tid >= o;
            if (have) left = s_scan[tid - o];
            __syncthreads();
            if (have) s_scan[tid] = cbw_compose(left, s_scan[tid]);
            __syncthreads();
        }
        if (tid == 0) { s_cross = 0xFFFFFFFFu; s_m = 0; }
        __syncthreads();
        // (3) this thread's start value, then its chunks one by one: the first chunk whose end value passes the limit
        {
            const cbw_map before = tid ? s_scan[tid - 1] : cbw_map{ 0u, 0u };
            uint64_t m = (uint64_t)m0 + ((m0 & 1u) ? before.d1 : before.d0);
            for (uint32_t c = max(c0, start); c < c1; c++) {
                const cbw_map mp = maps[c];
                const uint64_t end = m + ((m & 1u) ? mp.d1 : mp.d0);
                const bool crosses = exact_region ? end > (uint64_t)limit : end >= (uint64_t)limit;
                if (crosses) { atomicMin(&s_cross, c); break; }   // (chunks behind it are not looked at: their start values assumed this binade)
                m = end;
            }
        }
        __syncthreads();
        const uint32_t cross = s_cross;
        // (4) the value in front of the crossing chunk (or behind the last chunk): from the thread whose range holds that chunk (the last thread for the end of the list)
        {
            const uint32_t target = cross == 0xFFFFFFFFu ? n_chunks : cross;
            const bool holds = cross == 0xFFFFFFFFu ? (tid == (uint32_t)THREADS - 1u) : (target >= c0 && target < c1);
            if (holds) {
                const cbw_map before = tid ? s_scan[tid - 1] : cbw_map{ 0u, 0u };
                uint64_t m = (uint64_t)m0 + ((m0 & 1u) ? before.d1 : before.d0);
                for (uint32_t c = max(c0, start); c < min(c1, target); c++) { const cbw_map mp = maps[c]; m += (m & 1u) ? mp.d1 : mp.d0; }
                s_m = (uint32_t)m;   // < 2^24 (<= 2^24 in the exact region)
            }
        }
        __syncthreads();
        const float f_front = exact_region ? (float)s_m : __uint_as_float(((uint32_t)(e + 127) << 23) | (s_m & 0x7FFFFFu));   // m * u: m keeps the binade's exponent
        if (cross == 0xFFFFFFFFu) { if (tid == 0) s_f = f_front; __syncthreads(); start = n_chunks; break; }
        // (5) the crossing chunk, texel by texel with real adds
        {
            const uint32_t j0 = cross * CBW_SUM_CHUNK, j1 = min(j0 + CBW_SUM_CHUNK, n);
            for (uint32_t j = j0 + tid; j < j1; j += THREADS) s_vals[j - j0] = (float)value(j);
            __syncthreads();
            if (tid == 0) {
                float acc = f_front;
                for (uint32_t j = 0; j < j1 - j0; j++) acc += s_vals[j];
                s_f = acc;
            }
            __syncthreads();
        }
        start = cross + 1;
    }
    return s_f;
}

// ---------------------------------------------------------------------------------------------------------------- per-chunk passes
template <bool PERCEPTUAL, bool FORCED>
__global__ __launch_bounds__(256) void k_cbw_init(const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ indices, const cb_wide_chunk* __restrict__ chunks,
                                                  cb_wide_state* states, uint32_t step, const uint8_t* __restrict__ params, const uint8_t* __restrict__ valid,
                                                  const uint64_t* __restrict__ enc_blocks) {
    const cb_wide_chunk ch = chunks[blockIdx.x];
    cb_wide_state& st = states[ch.big];
    const uint32_t n = st.n_texels, ci = st.cluster;
    const uint32_t* members = indices + st.first;
    const uint32_t j1 = min(ch.first_texel + CBW_CHUNK, n);
    uint64_t sr = 0, sg = 0, sb = 0, prev = 0;
    int mn_r = 255, mn_g = 255, mn_b = 255, mx_r = 0, mx_g = 0, mx_b = 0;
    const bool with_prev = !FORCED && step != 0 && valid[ci] != 0;
    cvec pbc[4];
    if (with_prev) block_cvecs<PERCEPTUAL>(pbc, scale5(params[ci * 4 + 0]), scale5(params[ci * 4 + 1]), scale5(params[ci * 4 + 2]), params[ci * 4 + 3]);
    for (uint32_t j = ch.first_texel + threadIdx.x; j < j1; j += 256) {
        const uint32_t w = cluster_pixel(pixel_words, members, j);
        const int r = w & 255, g = (w >> 8) & 255, b = (w >> 16) & 255;
        sr += r; sg += g; sb += b;
        mn_r = min(mn_r, r); mn_g = min(mn_g, g); mn_b = min(mn_b, b);
        mx_r = max(mx_r, r); mx_g = max(mx_g, g); mx_b = max(mx_b, b);
        if (with_prev) prev += min_err4<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(w), pbc);
        if (FORCED) {   // the texel against the colour its own block's current encoding gives it (frontend.cpp:2773)
            const uint32_t tv = members[j >> 3];
            uint32_t r5, g5, b5, inten;
            unpack_etc1s_header(enc_blocks[tv >> 1], r5, g5, b5, inten);
            cvec bc[4];
            block_cvecs<PERCEPTUAL>(bc, scale5((int)r5), scale5((int)g5), scale5((int)b5), (int)inten);
            prev += cdist<PERCEPTUAL>(pixel_cvec<PERCEPTUAL>(w), select_cvec(bc, cluster_pixel_selector(enc_blocks, members, j)));
        }
    }
    sr = wave_allsum_u64(sr); sg = wave_allsum_u64(sg); sb = wave_allsum_u64(sb); prev = wave_allsum_u64(prev);
    mn_r = wave_min_i32(mn_r); mn_g = wave_min_i32(mn_g); mn_b = wave_min_i32(mn_b);
    mx_r = wave_max_i32(mx_r); mx_g = wave_max_i32(mx_g); mx_b = wave_max_i32(mx_b);
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&st.sum[0], (unsigned long long)sr); atomicAdd(&st.sum[1], (unsigned long long)sg); atomicAdd(&st.sum[2], (unsigned long long)sb);
        if (with_prev || FORCED) atomicAdd(&st.prev_tot, (unsigned long long)prev);
        atomicMin(&st.mn[0], mn_r); atomicMin(&st.mn[1], mn_g); atomicMin(&st.mn[2], mn_b);
        atomicMax(&st.mx[0], mx_r); atomicMax(&st.mx[1], mx_g); atomicMax(&st.mx[2], mx_b);
    }
}

template <int QUALITY>
__global__ __launch_bounds__(1024) void k_cbw_mean(const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ indices, cb_wide_state* states, cbw_map* sum_scratch) {
    cb_wide_state& st = states[blockIdx.x];
    const uint32_t n = st.n_texels;
    const uint32_t* members = indices + st.first;
    for (int c = 0; c < 3; c++) {
        const unsigned long long s = st.sum[c];
        float fs;
        if (s <= (1ull << 24)) fs = (float)s;   // every partial sum of the reference's running float sum is an exactly representable integer
        else fs = cbw_ordered_sum<1024>(pixel_words, members, n, st.n_sum_chunks, c, sum_scratch + st.sum_scratch_at);   // (uniform branch: s is the same for every thread)
        if (threadIdx.x == 0) st.avg[c] = fs / (float)n;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st.spread = max(max(st.mx[0] - st.mn[0], st.mx[1] - st.mn[1]), st.mx[2] - st.mn[2]);
        st.enable_mask = (QUALITY > BU_Q_MEDIUM) ? 0xFFu : (uint32_t)c_inten_enable_by_spread[st.spread];
        st.i = -2; st.active = 0; st.done = 0; st.best_err = ~0ull; st.best_r = st.best_g = st.best_b = st.best_inten = 0; st.best_valid = 0;
    }
}

// the serial part of etc1_optimizer::compute's trial loop (etc.cpp:948-1000): takes the totals of the trial in flight, prepares the next ACTIVE trial
template <int QUALITY>
__global__ __launch_bounds__(64) void k_cbw_step(cb_wide_state* states) {
    if (threadIdx.x != 0) return;
    cb_wide_state& st = states[blockIdx.x];
    if (st.done) return;
    const int perms = (int)perms_for_quality(QUALITY);
    const uint32_t enable_mask = st.enable_mask;
    unsigned long long best_err = st.best_err;
    int best_r = st.best_r, best_g = st.best_g, best_b = st.best_b, best_inten = st.best_inten, best_valid = st.best_valid;
    int i = st.i;
    bool done = false;
    if (st.active) {   // the trial that was just evaluated
        unsigned long long trial_err = (unsigned long long)INT64_MAX; // etc.cpp:1131
        int trial_inten = 0, trial_valid = 0;
        for (int t = 0; t < 8; t++) {
            if (!((enable_mask >> t) & 1u)) continue;
            const unsigned long long s = st.tot[t];
            if (s < trial_err) { trial_err = s; trial_inten = t; trial_valid = 1; }
        }
        if (trial_err < best_err) { best_err = trial_err; best_inten = trial_inten; best_valid = trial_valid; best_r = st.tr; best_g = st.tg; best_b = st.tb; }
        if (best_err == 0 || !best_valid) done = true;   // etc.cpp:955-956, 993-994: the end of iteration i
    }
    int tr = 0, tg = 0, tb = 0, active = 0;
    while (!done) {
        i = (i == -2) ? -1 : i + 1;
        if (i >= perms) { done = true; break; }
        bool a = true;
        if (i < 0) { tr = avg_to_color5(st.avg[0]); tg = avg_to_color5(st.avg[1]); tb = avg_to_color5(st.avg[2]); }
        else a = cluster_fit_trial(c_cluster_fit_order[i], best_r, best_g, best_b, best_inten, st.avg[0], st.avg[1], st.avg[2], tr, tg, tb);
        if (a) a = bloom_test_and_set(st.bloom, tr, tg, tb);
        if (a) { active = 1; break; }
        if (best_err == 0 || !best_valid) done = true;   // an iteration that evaluates nothing still ends with the loop's test
    }
    st.best_err = best_err; st.best_r = best_r; st.best_g = best_g; st.best_b = best_b; st.best_inten = best_inten; st.best_valid = best_valid;
    st.i = i; st.active = active; st.tr = tr; st.tg = tg; st.tb = tb; st.done = done ? 1 : 0;
    for (int t = 0; t < 8; t++) st.tot[t] = 0;
}

template <bool PERCEPTUAL, bool FORCED>
__global__ __launch_bounds__(256) void k_cbw_eval(const uint32_t* __restrict__ pixel_words, const uint32_t* __restrict__ indices, const cb_wide_chunk* __restrict__ chunks,
                                                  cb_wide_state* states, const uint64_t* __restrict__ enc_blocks) {
    const cb_wide_chunk ch = chunks[blockIdx.x];
    cb_wide_state& st = states[ch.big];
    if (st.done || !st.active) return;
    const uint32_t n = st.n_texels;
    const uint32_t* members = indices + st.first;
    const uint32_t j1 = min(ch.first_texel + CBW_CHUNK, n);
    const int tr = st.tr, tg = st.tg, tb = st.tb;
    const uint32_t enable_mask = st.enable_mask;
    cvec bc[8][4];
#pragma unroll
    for (int t = 0; t < 8; t++) block_cvecs<PERCEPTUAL>(bc[t], scale5(tr), scale5(tg), scale5(tb), t);
    uint64_t tot[8];
#pragma unroll
    for (int t = 0; t < 8; t++) tot[t] = 0;
    uint32_t plain_mask = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) plain_mask |= base_unclamped(scale5(tr), scale5(tg), scale5(tb), t) ? (1u << t) : 0u;
    plain_mask &= enable_mask;
    const cvec base_cv = to_cvec<PERCEPTUAL>(scale5(tr), scale5(tg), scale5(tb));
    for (uint32_t j = ch.first_texel + threadIdx.x; j < j1; j += 256) {
        const cvec p = pixel_cvec<PERCEPTUAL>(cluster_pixel(pixel_words, members, j));
        if (FORCED) {
            const uint32_t sel = cluster_pixel_selector(enc_blocks, members, j);
#pragma unroll
            for (int t = 0; t < 8; t++) tot[t] += cdist<PERCEPTUAL>(p, select_cvec(bc[t], sel));
        } else if (PERCEPTUAL && plain_mask) {
            const uint32_t chr = chroma_term(p.y - base_cv.y, p.z - base_cv.z);
            const int dx0 = p.x - base_cv.x;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                if (!((enable_mask >> t) & 1u)) continue;
                if ((plain_mask >> t) & 1u) tot[t] += min_luma_term(dx0, k_inten_a[t] * 64, k_inten_b[t] * 64) + chr;
                else tot[t] += min_err4<PERCEPTUAL>(p, bc[t]);
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
        if ((threadIdx.x & 63u) == 0 && s) atomicAdd(&st.tot[t], (unsigned long long)s);
    }
}

template <bool FORCED>
__global__ __launch_bounds__(64) void k_cbw_final(const cb_wide_state* __restrict__ states, uint32_t step, uint8_t* __restrict__ params, uint64_t* __restrict__ err_out,
                                                  uint8_t* __restrict__ valid, uint64_t* __restrict__ cur_err_out) {
    if (threadIdx.x != 0) return;
    const cb_wide_state& st = states[blockIdx.x];
    const uint32_t ci = st.cluster;
    if (FORCED) {
        cur_err_out[ci] = st.prev_tot;
        params[ci * 4 + 0] = (uint8_t)st.best_r; params[ci * 4 + 1] = (uint8_t)st.best_g; params[ci * 4 + 2] = (uint8_t)st.best_b; params[ci * 4 + 3] = (uint8_t)st.best_inten;
        err_out[ci] = st.best_err;
        valid[ci] = st.best_valid ? 1 : 0;
        return;
    }
    bool use_new = true;
    if (step != 0 && valid[ci]) use_new = st.prev_tot > st.best_err;   // keep the previous endpoints unless the error strictly drops (frontend.cpp:1554-1605)
    if (use_new) {
        params[ci * 4 + 0] = (uint8_t)st.best_r; params[ci * 4 + 1] = (uint8_t)st.best_g; params[ci * 4 + 2] = (uint8_t)st.best_b; params[ci * 4 + 3] = (uint8_t)st.best_inten;
        err_out[ci] = st.best_err;
        valid[ci] = 1;
    }
}

struct cb_wide_plan { const cb_wide_chunk* chunks; uint32_t n_chunks; cb_wide_state* states; uint32_t n_big; void* sum_scratch; };

template <bool P, int Q, bool F>
static void cbw_launch(hipStream_t st, const uint32_t* pw, const uint32_t* d_indices, const cb_wide_plan& pl, uint32_t step, uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid,
                       const uint64_t* enc, uint64_t* d_cur_err) {
    hipLaunchKernelGGL((k_cbw_init<P, F>), dim3(pl.n_chunks), dim3(256), 0, st, pw, d_indices, pl.chunks, pl.states, step, d_params, d_valid, enc);
    hipLaunchKernelGGL((k_cbw_mean<Q>), dim3(pl.n_big), dim3(1024), 0, st, pw, d_indices, pl.states, static_cast<cbw_map*>(pl.sum_scratch));
    hipLaunchKernelGGL((k_cbw_step<Q>), dim3(pl.n_big), dim3(64), 0, st, pl.states);
    const int rounds = (Q == BU_Q_FAST ? 4 : Q == BU_Q_MEDIUM ? 16 : Q == BU_Q_SLOW ? 64 : 165) + 1;   // = perms_for_quality + the trial at the mean colour
    for (int r = 0; r < rounds; r++) {
        hipLaunchKernelGGL((k_cbw_eval<P, F>), dim3(pl.n_chunks), dim3(256), 0, st, pw, d_indices, pl.chunks, pl.states, enc);
        hipLaunchKernelGGL((k_cbw_step<Q>), dim3(pl.n_big), dim3(64), 0, st, pl.states);
    }
    hipLaunchKernelGGL((k_cbw_final<F>), dim3(pl.n_big), dim3(64), 0, st, pl.states, step, d_params, d_err, d_valid, d_cur_err);
}

// ---------------------------------------------------------------------------------------------------------------- host side
// workspace = [states | chunk table | ordered-sum scratch]; the first two are made here (host image, uploaded by the caller), the third needs no initialisation
cb_wide_layout codebook_wide_prepare(const uint32_t* h_cluster, const uint32_t* h_first, const uint32_t* h_subblocks, uint32_t n_big, std::vector<unsigned char>& image) {
    cb_wide_layout L{};
    L.n_big = n_big;
    uint64_t n_chunks = 0, sum_entries = 0;
    for (uint32_t b = 0; b < n_big; b++) {
        const uint64_t texels = (uint64_t)h_subblocks[b] * 8u;
        n_chunks += (texels + CBW_CHUNK - 1) / CBW_CHUNK;
        sum_entries += (texels + CBW_SUM_CHUNK - 1) / CBW_SUM_CHUNK;
    }
    L.n_chunks = (uint32_t)n_chunks;
    L.states_at = 0;
    L.chunks_at = ((size_t)n_big * sizeof(cb_wide_state) + 255) & ~(size_t)255;
    L.sum_at = (L.chunks_at + (size_t)n_chunks * sizeof(cb_wide_chunk) + 255) & ~(size_t)255;
    L.total = L.sum_at + (size_t)sum_entries * sizeof(cbw_map);
    L.image_bytes = L.sum_at;
    image.assign(L.image_bytes, 0);
    cb_wide_state* st = reinterpret_cast<cb_wide_state*>(image.data() + L.states_at);
    cb_wide_chunk* ch = reinterpret_cast<cb_wide_chunk*>(image.data() + L.chunks_at);
    uint64_t sum_at = 0; size_t k = 0;
    for (uint32_t b = 0; b < n_big; b++) {
        const uint32_t texels = h_subblocks[b] * 8u;
        st[b].cluster = h_cluster[b]; st[b].first = h_first[b]; st[b].n_texels = texels; st[b].n_sum_chunks = (texels + CBW_SUM_CHUNK - 1) / CBW_SUM_CHUNK;
        st[b].sum_scratch_at = sum_at; sum_at += st[b].n_sum_chunks;
        for (int c = 0; c < 3; c++) { st[b].mn[c] = 255; st[b].mx[c] = 0; }
        for (uint32_t t = 0; t < texels; t += CBW_CHUNK) ch[k++] = cb_wide_chunk{ b, t };
    }
    return L;
}

// test hook: only the colour means (init + mean passes) of the clusters of a prepared workspace; d_out: 3 floats per large cluster, in the order of the preparation
__global__ __launch_bounds__(64) void k_cbw_read_means(const cb_wide_state* __restrict__ states, uint32_t n_big, float* __restrict__ out) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b < n_big) { out[b * 3 + 0] = states[b].avg[0]; out[b * 3 + 1] = states[b].avg[1]; out[b * 3 + 2] = states[b].avg[2]; }
}
hipError_t launch_codebook_wide_means(hipStream_t st, const void* d_pixel_blocks, const uint32_t* d_indices, void* d_work, const cb_wide_layout& L, float* d_out) {
    if (!L.n_big) return hipSuccess;
    char* base = static_cast<char*>(d_work);
    cb_wide_state* states = reinterpret_cast<cb_wide_state*>(base + L.states_at);
    const uint32_t* pw = static_cast<const uint32_t*>(d_pixel_blocks);
    hipLaunchKernelGGL((k_cbw_init<true, false>), dim3(L.n_chunks), dim3(256), 0, st, pw, d_indices, reinterpret_cast<const cb_wide_chunk*>(base + L.chunks_at), states, 0u,
                       (const uint8_t*)nullptr, (const uint8_t*)nullptr, (const uint64_t*)nullptr);
    hipLaunchKernelGGL((k_cbw_mean<BU_Q_MEDIUM>), dim3(L.n_big), dim3(1024), 0, st, pw, d_indices, states, reinterpret_cast<cbw_map*>(base + L.sum_at));
    hipLaunchKernelGGL(k_cbw_read_means, dim3((L.n_big + 63) / 64), dim3(64), 0, st, states, L.n_big, d_out);
    return hipGetLastError();
}

hipError_t launch_codebook_wide(hipStream_t st, const void* d_pixel_blocks, const uint32_t* d_indices, void* d_work, const cb_wide_layout& L, int quality, bool perceptual, bool forced,
                                uint32_t step, const void* d_enc_blocks, uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint64_t* d_cur_err) {
    if (!L.n_big) return hipSuccess;
    char* base = static_cast<char*>(d_work);
    const cb_wide_plan pl{ reinterpret_cast<const cb_wide_chunk*>(base + L.chunks_at), L.n_chunks, reinterpret_cast<cb_wide_state*>(base + L.states_at), L.n_big, base + L.sum_at };
    const uint32_t* pw = static_cast<const uint32_t*>(d_pixel_blocks);
    const uint64_t* enc = static_cast<const uint64_t*>(d_enc_blocks);
    if (quality < BU_Q_MEDIUM) quality = BU_Q_MEDIUM;   // (as the one-workgroup launches)
    with_bool(perceptual, [&](auto p) { with_bool(forced, [&](auto f) { with_quality<BU_Q_MEDIUM>(quality, [&](auto q) {
        cbw_launch<decltype(p)::value, decltype(q)::value, decltype(f)::value>(st, pw, d_indices, pl, step, d_params, d_err, d_valid, enc, d_cur_err);
    }); }); });
    return hipGetLastError();
}
