// host/ssim.cpp -- bu_ssim_gaussian_weights (include/basisu_hip_image_metrics.h): ssim_gaussian_weights of ../ssim.h behind the C ABI of libbasisu_frontend.so.
#include "../../../include/basisu_hip_image_metrics.h"
#include "../ssim.h"

extern "C" int bu_ssim_gaussian_weights(float out[121]) {
    if (!out) return 0;
    bu::ssim_gaussian_weights(out);
    return 1;
}
