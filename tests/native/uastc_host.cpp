// tests/native/uastc_host.cpp -- TEST INFRASTRUCTURE ONLY: the UASTC device core (basis_universal_amd/csrc/uastc_core.h) compiled
// for the host with g++, so that every stage can be diffed against the real reference (oracle/_ref) on the CPU, where there is
// no GPU. The product never builds or loads this file; libbasisu_hip.so compiles the same header with hipcc.
#include <cstring>
#include <map>
#include <vector>
#include <utility>
#include "../../basis_universal_amd/csrc/uastc_rdo.h"
#include "host_api.h"

using namespace bu_uastc;

// `mask` selects the texels of the 16 given ones that form the cell (the reference sees them gathered, in the same order)
HOST_API uint64_t hc_cell_compress(const uint8_t* px16, uint32_t mask, uint32_t wbits, uint32_t range, int alpha, uint32_t uber, uint32_t ls_passes, uint8_t* out24) {
    cell_cfg cfg;
    cfg.wbits = (uint8_t)wbits; cfg.range = (uint8_t)range; cfg.alpha = (uint8_t)alpha; cfg.uber = (uint8_t)uber; cfg.ls_passes = (uint8_t)ls_passes; cfg.ls_weights = ku_weights_ls + ((1u << wbits) - 2u) * 4;
    uint32_t px[16];
    for (int i = 0; i < 16; i++) px[i] = pack_px(px16 + i * 4);
    cell_fit f;
    memset(&f, 0, sizeof(f));
    const uint64_t e = cell_compress(px, mask, cfg, f);
    memcpy(out24, f.astc_lo, 4); memcpy(out24 + 4, f.astc_hi, 4);
    for (int i = 0; i < 16; i++) out24[8 + i] = (uint8_t)sel_get(f.sel, i);
    return e;
}
HOST_API uint64_t hc_cell_estimate(uint32_t wbits, uint32_t comps, const uint8_t* px16, uint32_t mask) {
    uint32_t px[16];
    for (int i = 0; i < 16; i++) px[i] = pack_px(px16 + i * 4);
    return estimate_masked_any(wbits, comps, px, mask);
}
HOST_API uint32_t hc_weight_of(uint32_t bits, uint32_t s) { return weight_of(bits, s); }
HOST_API uint32_t hc_weight_table(uint32_t bits, uint32_t s) { return weight_set(bits)[s]; }

HOST_API void hc_encode_uastc(const uint8_t* blocks, uint32_t n, uint32_t flags, uint8_t* out) {
    static cand scratch[MAX_SLOTS];
    for (uint32_t i = 0; i < n; i++) encode_block(blocks + (size_t)i * 64, flags, out + (size_t)i * 16, scratch);
}

// uastc_rdo (uastc_enc.cpp:3824-4163) as a scalar loop over the shared per-block pieces of uastc_rdo.h: the order-defining part of the
// GPU strips kernel (history of selector fields, window scan newest-first, strict "<" on the cost) restated the plain way.
static bool g_table_trials = false;  // score trials from the per-block error table (what the GPU strips kernel does) instead of decoding them
// counts (may be null): [0] walks that replaced a block's selectors, [1] refits that changed a block, [2] blocks rdo_prepare says to skip: what k_rdo_strips,
// settle_window and k_rdo_finish count on the device
static bool rdo_strip(uint32_t first, uint32_t last, uint8_t* blocks, const uint8_t* pixels, const rdo_params& p, uint32_t flags, uint32_t* counts = nullptr) {
    uint32_t none[3] = { 0, 0, 0 };
    if (!counts) counts = none;
    enc_cfg e;
    make_cfg(flags, e);
    const int window = (int)(p.lz_dict_size / 16 > 1 ? p.lz_dict_size / 16 : 1);
    std::map<std::pair<uint32_t, uint64_t>, uint32_t> history;
    std::vector<uint8_t> state(last - first, 0);  // 1: modified, refit pending; 2: modified, only the hints are stale
    for (uint32_t i = first; i < last; i++) {
        uint8_t* blk = blocks + (size_t)i * 16;
        const rgba8* px = (const rgba8*)(pixels + (size_t)i * 64);
        cand cur;
        rdo_block_info info;
        if (!rdo_prepare(blk, px, p, cur, info)) return false;
        if (info.mode == 8) continue;
        if (g_table_trials && rdo_mode_reads_endpoint_bits(info.mode)) {
            const int from = (int)i - window > (int)first ? (int)i - window : (int)first;
            for (int j = from; j < (int)i; j++)
                if (state[j - first] == 1) {
                    bool refined;
                    if (!rdo_refit_block((const rgba8*)(pixels + (size_t)j * 64), p, blocks + (size_t)j * 16, refined)) return false;
                    counts[1] += refined ? 1u : 0u;
                    state[j - first] = 2;
                }
        }
        const uint32_t fsb = ku_sel_first[info.mode], len = ku_sel_len[info.mode], len_lo = len < 64 ? len : 64;
        const uint64_t cur_lo = block_bits(blk, fsb, len_lo);
        if (info.skip) { counts[2]++; history[{ fsb, cur_lo }] = i; continue; }
        int cur_bits;
        auto it = history.find({ fsb, cur_lo });
        if (it == history.end()) cur_bits = (int)((len * p.lz_literal_cost) / 100);
        else cur_bits = (int)match_cost((i - it->second) * 16);
        uint32_t table[RDO_TABLE_WORDS];
        uint32_t amask = 0;
        if (g_table_trials) {
            texel_ends ends;
            rdo_texel_ends(cur, ends);
            amask = rdo_anchor_mask(cur.mode, cur.pattern);
            const uint32_t planes = ku_mode_planes[cur.mode];
            for (uint32_t k = 0; k < 16 * planes; k++)
                for (uint32_t v = 0; v < (1u << ku_mode_weight_bits[cur.mode]); v++)
                    table[(k << ku_mode_weight_bits[cur.mode]) + v] = rdo_weight_error(cur.mode, cur.ccs, k, v, ends.ul[k / planes], ends.uh[k / planes], ends.bl[k / planes], ends.bh[k / planes],
                                                         pack_px(px[k / planes].c));
        }
        float best_t = info.ms_err * info.scale + (float)cur_bits * p.lambda;
        int best_j = -1;
        uint64_t best_lo = 0, best_hi = 0;
        const int lo_j = (int)i - window > (int)first ? (int)i - window : (int)first;
        for (int j = (int)i - 1; j >= lo_j; j--) {
            const uint8_t* prev = blocks + (size_t)j * 16;
            const uint64_t lo = block_bits(prev, fsb, len_lo), hi = len > 64 ? block_bits(prev, fsb + 64, len - 64) : 0;
            int match = j;
            auto f = history.find({ fsb, lo });
            if (f != history.end()) match = (int)f->second;
            if (match > j) continue;
            cand tmp;
            if (!unpack_block(prev, tmp)) return false;
            float ms;
            if (g_table_trials) {
                ms = (float)(uint64_t)(rdo_trial_sum(table, cur.mode, amask, lo, hi) / 2) * (1.0f / 64.0f);
                if (sqrtf(ms) > info.rms_err * p.max_allowed_rms_increase_ratio) continue;
            } else if (!rdo_trial(cur, lo, hi, px, info, p, ms)) continue;
            const float t = ms * info.scale + (float)(int)match_cost((i - (uint32_t)match) * 16) * p.lambda;
            if (t < best_t) { best_t = t; best_j = j; best_lo = lo; best_hi = hi; }
        }
        uint64_t final_lo = cur_lo;
        if (best_j >= 0) {
            counts[0]++;
            if (g_table_trials) {  // the GPU schedule: raw trial bits now, refit + hints later (uastc_rdo.h, "Deferred form")
                put_field(blk, fsb, len, best_lo, best_hi);
                state[i - first] = (p.endpoint_refinement && info.mode == 0) ? 1 : 2;
            } else {
                bool refined;
                rdo_write_back(cur, best_lo, best_hi, px, p, blk, refined);
                counts[1] += refined ? 1u : 0u;
                if (!rdo_rehint(px, e, blk)) return false;
            }
            final_lo = block_bits(blk, fsb, len_lo);
        }
        history[{ fsb, final_lo }] = i;
    }
    for (uint32_t i = first; i < last; i++) {
        if (!state[i - first]) continue;
        const rgba8* px = (const rgba8*)(pixels + (size_t)i * 64);
        bool refined;
        if (state[i - first] == 1) {
            if (!rdo_refit_block(px, p, blocks + (size_t)i * 16, refined)) return false;
            counts[1] += refined ? 1u : 0u;
        }
        if (!rdo_rehint(px, e, blocks + (size_t)i * 16)) return false;
    }
    return true;
}

// hc_uastc_rdo plus the three counters of bu_hip_k_uastc_rdo's out_stats: modified, refined, skipped (summed over the strips)
HOST_API int hc_uastc_rdo_counted(uint8_t* blocks, const uint8_t* pixels, uint32_t n, const float* fp, const uint32_t* up, uint32_t flags, uint32_t total_jobs, uint32_t* counts3) {
    g_table_trials = (total_jobs >> 31) != 0;  // test switch in the top bit
    total_jobs &= 0x7FFFFFFFu;
    rdo_params p;
    p.lambda = fp[0]; p.max_allowed_rms_increase_ratio = fp[1]; p.skip_block_rms_thresh = fp[2]; p.max_smooth_block_std_dev = fp[3];
    p.smooth_block_max_error_scale = fp[4];
    p.lz_dict_size = up[0]; p.lz_literal_cost = up[1]; p.endpoint_refinement = up[2];
    const uint32_t per_job = total_jobs ? n / total_jobs : 0;
    counts3[0] = counts3[1] = counts3[2] = 0;
    if (total_jobs <= 1 || per_job <= 8) return rdo_strip(0, n, blocks, pixels, p, flags, counts3) ? 1 : 0;
    for (uint32_t f = 0; f < n; f += per_job)
        if (!rdo_strip(f, f + per_job < n ? f + per_job : n, blocks, pixels, p, flags, counts3)) return 0;
    return 1;
}
HOST_API int hc_uastc_rdo(uint8_t* blocks, const uint8_t* pixels, uint32_t n, const float* fp, const uint32_t* up, uint32_t flags, uint32_t total_jobs) {
    uint32_t counts[3];
    return hc_uastc_rdo_counted(blocks, pixels, n, fp, up, flags, total_jobs, counts);
}

HOST_API int hc_unpack_block(const uint8_t* blk, uint8_t* out64) {
    cand c;
    const bool ok = unpack_block(blk, c);
    memcpy(out64, &c, 64);
    return ok ? 1 : 0;
}

// whole decoder: 16-byte UASTC blocks -> 4x4 RGBA texels (unpack_uastc + the per-texel interpolation of the core: what a transcoder to RGBA32 yields)
HOST_API int hc_decode_uastc(const uint8_t* blocks, uint32_t n, uint8_t* out_rgba64) {
    for (uint32_t i = 0; i < n; i++) {
        cand c;
        if (!unpack_block(blocks + (size_t)i * 16, c)) return 0;
        rgba8* o = reinterpret_cast<rgba8*>(out_rgba64 + (size_t)i * 64);
        if (c.mode == 8) { for (int t = 0; t < 16; t++) for (int k = 0; k < 4; k++) o[t].c[k] = c.endpoints[k]; }   // solid colour: the four bytes are the texel
        else decode_uastc(c, o);
    }
    return 1;
}

HOST_API int hc_rehint(const uint8_t* pixels, uint32_t n, uint32_t flags, uint8_t* blocks) {
    enc_cfg e;
    make_cfg(flags, e);
    for (uint32_t i = 0; i < n; i++)
        if (!rdo_rehint((const rgba8*)(pixels + (size_t)i * 64), e, blocks + (size_t)i * 16)) return 0;
    return 1;
}

// every candidate of every block: the fused decode + error (uastc_errors / bc7_errors, what score_candidate uses) against the general decoders + block_error
HOST_API uint32_t hc_score_selfcheck(const uint8_t* blocks, uint32_t n, uint32_t flags, uint32_t* checked) {
    enc_cfg e;
    make_cfg(flags, e);
    uint32_t bad = 0, seen = 0;
    static cand slots[MAX_SLOTS];
    for (uint32_t i = 0; i < n; i++) {
        const rgba8* px = (const rgba8*)(blocks + (size_t)i * 64);
        const uint32_t cls = classify(px, e);
        if (cls & CLS_SOLID) continue;
        uint32_t packed[16];
        for (int k = 0; k < 16; k++) packed[k] = pack_px(px[k].c);
        for (uint32_t m = 0; m < 19; m++) {
            const uint32_t nv = mode_variants(m, e);
            if (!nv || !mode_applies(m, cls, e)) continue;
            for (uint32_t v = 0; v < nv; v += (e.estimate_partition && (m == 9 || m == 16)) ? nv : 1) {
                cand out[4];
                const uint32_t cnt = (e.estimate_partition && (m == 9 || m == 16)) ? nv : 1;
                run_mode(m, px, e, out, v, cnt);
                for (uint32_t k = 0; k < cnt; k++) {
                    rgba8 du[16], db[16];
                    decode_uastc(out[k], du);
                    decode_bc7(out[k], db);
                    const block_err eu = block_error(px, du), eb = block_error(px, db);
                    chan_err cu, cb;
                    uastc_errors(out[k], packed, cu);
                    bc7_errors(out[k], packed, cb);
                    const block_err fu = chan_err_totals(cu), fb = chan_err_totals(cb);
                    seen++;
                    if (eu.rgb != fu.rgb || eu.rgba != fu.rgba || eu.la != fu.la || eb.rgb != fb.rgb || eb.rgba != fb.rgba || eb.la != fb.la) bad++;
                }
            }
        }
    }
    (void)slots;
    if (checked) *checked = seen;
    return bad;
}
