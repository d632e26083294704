// psnr_hvs_host.cpp -- TEST-ONLY host build of csrc/psnr_hvs.h: the per-block arithmetic the kernel's lanes share out, under a serial loop over two rasters.
// Built and bound by tests/native_libs.py.
#include <cstdint>
#include <cstring>

#include "../../basis_universal_amd/csrc/psnr_hvs.h"
#include "host_api.h"

// a, b: RGBA8 rasters, pitches in pixels; the region is min(wa, wb) x min(ha, hb), cut into 8x8 blocks whose coordinates are clamped to each raster's own edge.
// out_blocks[block * 2 + 0 / 1]: the HVS / HVS-M double of every block of `mode` (its 64 terms added in index order), blocks in raster order.
// running[0 / 1]: every term of every block added to ONE double in raster order, as psnr_hvs_compute_chan does. Returns the number of blocks.
HOST_API uint32_t phh_blocks(const uint8_t* a, uint32_t wa, uint32_t ha, uint32_t pitch_a, const uint8_t* b, uint32_t wb, uint32_t hb, uint32_t pitch_b, uint32_t mode,
                    double* out_blocks, double* running) {
    const uint32_t w = wa < wb ? wa : wb, h = ha < hb ? ha : hb;
    running[0] = running[1] = 0.0;
    if (!w || !h) return 0;
    const uint32_t bxs = (w + 7) / 8, bys = (h + 7) / 8;
    for (uint32_t by = 0; by < bys; by++)
        for (uint32_t bx = 0; bx < bxs; bx++) {
            uint32_t pa[64], pb[64];
            for (uint32_t i = 0; i < 64; i++) {
                const uint32_t x = bx * 8 + (i & 7), y = by * 8 + (i >> 3);
                memcpy(&pa[i], a + ((size_t)(y < ha ? y : ha - 1) * pitch_a + (x < wa ? x : wa - 1)) * 4, 4);
                memcpy(&pb[i], b + ((size_t)(y < hb ? y : hb - 1) * pitch_b + (x < wb ? x : wb - 1)) * 4, 4);
            }
            float th[64], tm[64];
            bu::hvs_block(mode, pa, pb, th, tm);
            double* o = out_blocks + (size_t)(by * bxs + bx) * 2;
            o[0] = bu::hvs_sum_terms(th);
            o[1] = bu::hvs_sum_terms(tm);
            for (uint32_t i = 0; i < 64; i++) {
                running[0] += (double)th[i];
                running[1] += (double)tm[i];
            }
        }
    return bxs * bys;
}

// sum_hvs[6], sum_hvsm[6], blocks -> out32: y_601_8bit, y_601_float, r, g, b, a, rgb, rgba, each mseh_hvs, mseh_hvsm, psnr_hvs, psnr_hvsm
HOST_API void phh_reduce(const double* sum_hvs, const double* sum_hvsm, uint32_t blocks, double* out32) {
    const bu::hvs_result r = bu::hvs_reduce(sum_hvs, sum_hvsm, blocks);
    const bu::hvs_chan all[8] = {r.y_601_8bit, r.y_601_float, r.chan[0], r.chan[1], r.chan[2], r.chan[3], r.rgb, r.rgba};
    for (int k = 0; k < 8; k++) {
        out32[k * 4 + 0] = all[k].mseh_hvs; out32[k * 4 + 1] = all[k].mseh_hvsm; out32[k * 4 + 2] = all[k].psnr_hvs; out32[k * 4 + 3] = all[k].psnr_hvsm;
    }
}
