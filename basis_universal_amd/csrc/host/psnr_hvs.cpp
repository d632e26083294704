// host/psnr_hvs.cpp -- bu_psnr_hvs_reduce (include/basisu_hip_image_metrics.h): hvs_reduce of ../psnr_hvs.h behind the C ABI of libbasisu_frontend.so.
#include "../../../include/basisu_hip_image_metrics.h"
#include "../psnr_hvs.h"
#include <cstddef>

extern "C" int bu_psnr_hvs_reduce(const bu_psnr_hvs_sums* sums, bu_psnr_hvs_metrics* out) {
    if (!sums || !out || sums->struct_bytes < offsetof(bu_psnr_hvs_sums, sum_hvsm) + sizeof(sums->sum_hvsm)) return 0;
    const bu::hvs_result r = bu::hvs_reduce(sums->sum_hvs, sums->sum_hvsm, sums->blocks);
    auto put = [](bu_psnr_hvs_chan& d, const bu::hvs_chan& s) { d.mseh_hvs = s.mseh_hvs; d.mseh_hvsm = s.mseh_hvsm; d.psnr_hvs = s.psnr_hvs; d.psnr_hvsm = s.psnr_hvsm; };
    put(out->y_601_8bit, r.y_601_8bit);
    put(out->y_601_float, r.y_601_float);
    for (int c = 0; c < 4; c++) put(out->chan[c], r.chan[c]);
    put(out->rgb, r.rgb);
    put(out->rgba, r.rgba);
    return 1;
}
