// host/image_metrics.cpp -- bu_image_metrics_reduce (include/basisu_hip_image_metrics.h): im_reduce of ../image_metrics.h behind the C ABI of libbasisu_frontend.so.
#include "../../../include/basisu_hip_image_metrics.h"
#include "../image_metrics.h"

extern "C" int bu_image_metrics_reduce(const uint32_t* hist, uint32_t total_chans, uint32_t first_chan, uint32_t width, uint32_t height, int use_601, bu_image_metrics* out) {
    if (!hist || !out || first_chan >= 4 || total_chans > 4 || first_chan + total_chans > 4) return 0;
    const bu::im_result r = bu::im_reduce(hist, total_chans, first_chan, width, height, use_601 != 0);
    out->max = r.max; out->mean = r.mean; out->mean_squared = r.mean_squared; out->rms = r.rms; out->psnr = r.psnr;
    return 1;
}
