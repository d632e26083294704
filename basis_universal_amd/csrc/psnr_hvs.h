// psnr_hvs.h -- the per-block arithmetic of psnr_hvs_compute_chan (encoder/basisu_enc.cpp:2256-2465) and the reduction of psnr_hvs_compute_metrics (:2467-2519), stated
// once for the kernel (psnr_hvs_kernels.hip), the host library (host/psnr_hvs.cpp, the reduction only) and the native test (tests/native/psnr_hvs_host.cpp). Compiles
// with and without hipcc; under hipcc the per-block pieces are device functions (their tables are device constants), as in uastc_core.h.
//
// Everything up to the per-coefficient terms is binary32 in the reference's operation order: build with -ffp-contract=off; sqrtf and / are IEEE on both sides. A block
// of one mode is 64 samples of each image -> two 8x8 DCTs -> two masking strengths -> 64 HVS terms and 64 HVS-M terms (floats) -> two doubles, the terms added in
// index order. The pieces are small enough to be called by one serial loop (hvs_block, the host) or by the lanes of a wave (the kernel: one lane per coefficient,
// one lane per order-fixed chain); both orders of calling them give the same bits because every float chain below is inside one function.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BU_HVS_FN __device__ inline
#define BU_HVS_TAB static __device__ const
#else
#define BU_HVS_FN static inline
#define BU_HVS_TAB static const
#endif

#include "psnr_hvs_tables.inc"

namespace bu {

// the six modes, in the order of bu_psnr_hvs_sums (include/basisu_hip.h)
enum : uint32_t { HVS_Y_8BIT = 0, HVS_Y_FLOAT = 1, HVS_R = 2, HVS_G = 3, HVS_B = 4, HVS_A = 5, HVS_MODES = 6 };

// one sample of a block; p: r | g << 8 | b << 16 | a << 24. BT.601 "studio swing" Y, rounded to 8 bits first (get_psnr_hvs_601_y) or kept in float
// (get_psnr_hvs_601_yf), enc.h:3912-3922; left-to-right association as written there.
BU_HVS_FN float hvs_sample(uint32_t mode, uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    if (mode == HVS_Y_8BIT) {
        const float y = 16.0f + 65.481f * (float)r * (1.0f / 255.0f) + 128.553f * (float)g * (1.0f / 255.0f) + 24.966f * (float)b * (1.0f / 255.0f);
        return (float)(uint8_t)roundf(y) * (1.0f / 255.0f);   // 16 <= y <= 235: the narrowing never wraps
    }
    if (mode == HVS_Y_FLOAT) return (16.0f + (65.481f / 255.0f) * (float)r + (128.553f / 255.0f) * (float)g + (24.966f / 255.0f) * (float)b) * (1.0f / 255.0f);
    return (float)((p >> (8 * (mode - HVS_R))) & 255u) * (1.0f / 255.0f);
}

// dct2f::forward (transcoder/basisu_transcoder.cpp:26680-26721), one output each. Horizontal pass: frequency v of row `row` of the block; vertical pass: frequency u of
// column v of the horizontal pass's result. A sum started at 0 over index 0..7, then scaled.
BU_HVS_FN float hvs_dct_horizontal(const float* block, uint32_t row, uint32_t v) {
    float s = 0.0f;
    for (uint32_t y = 0; y < 8; y++) s += block[row * 8 + y] * HVS_COS[v * 8 + y];
    return s * HVS_ALPHA[v != 0];
}
BU_HVS_FN float hvs_dct_vertical(const float* work, uint32_t u, uint32_t v) {
    float s = 0.0f;
    for (uint32_t x = 0; x < 8; x++) s += work[x * 8 + v] * HVS_COS[u * 8 + x];
    return s * HVS_ALPHA[u != 0];
}

// vari_ddof1_times_n (enc.cpp:2289-2310) over a w x w window of the block at (x0, y0), rows first: w = 8 is the whole block, w = 4 a quadrant
BU_HVS_FN float hvs_variance(const float* block, uint32_t x0, uint32_t y0, uint32_t w) {
    const uint32_t n = w * w;
    float mean = 0.0f;
    for (uint32_t y = 0; y < w; y++)
        for (uint32_t x = 0; x < w; x++) mean += block[(y0 + y) * 8 + (x0 + x)];
    mean /= (float)n;
    float sum_sq = 0.0f;
    for (uint32_t y = 0; y < w; y++)
        for (uint32_t x = 0; x < w; x++) {
            const float d = block[(y0 + y) * 8 + (x0 + x)] - mean;
            sum_sq += d * d;
        }
    return sum_sq * ((float)n / (float)(n - 1));
}

// the five variances of compute_mask_strength in the order it needs them: 0 = the block, 1-4 = the quadrants at (0,0), (4,0), (0,4), (4,4)
BU_HVS_FN float hvs_variance_k(const float* block, uint32_t k) {
    const uint32_t q = k ? k - 1 : 0;   // one call with run-time bounds: lanes of a wave that take different k stay in one loop
    return hvs_variance(block, (q & 1) * 4, (q >> 1) * 4, k ? 4 : 8);
}

// compute_mask_strength (enc.cpp:2327-2341): the weighted energy of the AC coefficients ...
BU_HVS_FN float hvs_mask_energy(const float* dct) {
    float mask = 0.0f;
    for (uint32_t i = 1; i < 64; i++) mask += (dct[i] * dct[i]) * HVS_MASK[i];
    return mask;
}
// ... and what it makes of it and the five variances var[0..4] (hvs_variance_k)
BU_HVS_FN float hvs_mask_strength(float energy, const float* var) {
    float pop = var[0];
    if (pop != 0.0f) {
        const float qsum = var[1] + var[2] + var[3] + var[4];
        pop = qsum / pop;
    }
    return sqrtf(energy * pop / 16.0f / 64.0f);
}

// coefficient i of both DCTs and the larger of the two masking strengths -> the HVS and the HVS-M term (enc.cpp:2425-2448), floats the caller widens
BU_HVS_FN void hvs_terms(float a_dct, float b_dct, uint32_t i, float mask, float* hvs, float* hvsm) {
    float u = fabsf(a_dct - b_dct);
    const float w = u * HVS_CSF[i];
    *hvs = w * w;
    if (i != 0) {
        const float threshold = mask / HVS_MASK[i];
        u = u < threshold ? 0.0f : u - threshold;
    }
    const float wm = u * HVS_CSF[i];
    *hvsm = wm * wm;
}

// 64 terms -> the block's double: added in index order
BU_HVS_FN double hvs_sum_terms(const float* terms) {
    double s = 0.0;
    for (uint32_t i = 0; i < 64; i++) s += (double)terms[i];
    return s;
}

// One block of one mode under a serial loop: pa / pb = the 64 pixels of the block in each image (extract_block_clamped), terms_* = the 64 float terms.
BU_HVS_FN void hvs_block(uint32_t mode, const uint32_t* pa, const uint32_t* pb, float* terms_hvs, float* terms_hvsm) {
    float blk[2][64], work[64], dct[2][64], strength[2];
    for (uint32_t img = 0; img < 2; img++) {
        const uint32_t* p = img ? pb : pa;
        for (uint32_t i = 0; i < 64; i++) blk[img][i] = hvs_sample(mode, p[i]);
        for (uint32_t i = 0; i < 64; i++) work[i] = hvs_dct_horizontal(blk[img], i >> 3, i & 7);
        for (uint32_t i = 0; i < 64; i++) dct[img][i] = hvs_dct_vertical(work, i >> 3, i & 7);
        float var[5];
        for (uint32_t k = 0; k < 5; k++) var[k] = hvs_variance_k(blk[img], k);
        strength[img] = hvs_mask_strength(hvs_mask_energy(dct[img]), var);
    }
    const float mask = strength[1] > strength[0] ? strength[1] : strength[0];
    for (uint32_t i = 0; i < 64; i++) hvs_terms(dct[0][i], dct[1][i], i, mask, &terms_hvs[i], &terms_hvsm[i]);
}

// ---- the reduction: host code on both compilers (plain doubles, no tables)

struct hvs_chan { double mseh_hvs, mseh_hvsm, psnr_hvs, psnr_hvsm; };
struct hvs_result { hvs_chan y_601_8bit, y_601_float, chan[4], rgb, rgba; };

// psnr_hvs_calc_psnr(mseh, 1.0) (enc.h:3902-3908): 10.0f * log10((1 * 1) / mseh) in double, 100000 for mseh <= 0
inline double hvs_psnr(double mseh) { return mseh <= 0.0 ? 100000.0 : 10.0 * log10(1.0 / mseh); }

// sum_hvs / sum_hvsm[HVS_MODES]: the sums over all blocks; psnr_hvs_compute_chan's tail (enc.cpp:2455-2462) per mode, then psnr_hvs_compute_metrics' averages
inline hvs_result hvs_reduce(const double* sum_hvs, const double* sum_hvsm, uint32_t blocks) {
    const uint32_t total_samples = blocks * 64;
    auto chan = [&](uint32_t mode) {
        hvs_chan c;
        c.mseh_hvs = sum_hvs[mode] / double(total_samples);
        c.mseh_hvsm = sum_hvsm[mode] / double(total_samples);
        c.psnr_hvs = hvs_psnr(c.mseh_hvs);
        c.psnr_hvsm = hvs_psnr(c.mseh_hvsm);
        return c;
    };
    hvs_result r;
    r.y_601_8bit = chan(HVS_Y_8BIT);
    r.y_601_float = chan(HVS_Y_FLOAT);
    double hvs_rgb = 0, hvsm_rgb = 0, hvs_rgba = 0, hvsm_rgba = 0;
    for (uint32_t c = 0; c < 4; c++) {
        r.chan[c] = chan(HVS_R + c);
        if (c < 3) {
            hvs_rgb += r.chan[c].mseh_hvs;
            hvsm_rgb += r.chan[c].mseh_hvsm;
        }
        hvs_rgba += r.chan[c].mseh_hvs;
        hvsm_rgba += r.chan[c].mseh_hvsm;
    }
    hvs_rgb /= 3.0f; hvsm_rgb /= 3.0f;
    hvs_rgba /= 4.0f; hvsm_rgba /= 4.0f;
    r.rgb = {hvs_rgb, hvsm_rgb, hvs_psnr(hvs_rgb), hvs_psnr(hvsm_rgb)};
    r.rgba = {hvs_rgba, hvsm_rgba, hvs_psnr(hvs_rgba), hvs_psnr(hvsm_rgba)};
    return r;
}

}  // namespace bu
