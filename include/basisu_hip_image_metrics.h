/* include/basisu_hip_image_metrics.h -- the float half of image_metrics::calc (encoder/basisu_enc.cpp:2205-2225): the counts of bu_hip_k_image_metrics
 * (basisu_hip.h) -> Max / Mean / RMS / PSNR as `basisu -stats` prints them per slice. Host code, lives in libbasisu_frontend.so
 * (basis_universal_amd/csrc/host/image_metrics.cpp over csrc/image_metrics.h); needs no GPU.
 *
 * The reference's expression order: 256 bins in ascending order, sum += i * h[i] and sum2 += i * (i * h[i]) in double; mean, mean_squared and rms narrowed to float;
 * psnr = rms ? clamp(log10(255.0 / rms) * 20, 0, 100) : 100; avg_comp_error = true as basis_compressor calls it (the divisor is width * height * channels).
 * This overload of calc never sets m_ssim; SSIM is bu_hip_k_ssim (basisu_hip.h), whose filter weights bu_ssim_gaussian_weights below computes.
 */
#ifndef BASISU_HIP_IMAGE_METRICS_H
#define BASISU_HIP_IMAGE_METRICS_H
#include "basisu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bu_image_metrics {
    double max;                                /* m_max: the largest difference that occurs */
    float mean, mean_squared, rms, psnr;
} bu_image_metrics;

/* hist: bu_image_metrics_counts::hist, 6 x 256. total_chans 1..4: channels first_chan .. first_chan + total_chans - 1 counted into one histogram (RGB Avg = 3 from 0,
 * RGBA Avg = 4 from 0, a single channel = 1 from its index); total_chans 0: a luma row, 601 when use_601 is set, else 709. Returns 0 (and leaves *out alone) on a null
 * pointer or a channel range past 4. */
BU_HIP_API int bu_image_metrics_reduce(const uint32_t* hist, uint32_t total_chans, uint32_t first_chan, uint32_t width, uint32_t height, int use_601, bu_image_metrics* out);

/* psnr_hvs_compute_metrics from its block sums on (encoder/basisu_enc.cpp:2455-2462, 2481-2514): the sums of bu_hip_k_psnr_hvs -> what psnr_hvs_print_metrics prints.
 * Per mode mseh = sum / double(blocks * 64) and psnr = 10.0f * log10(1 / mseh) in double, 100000 where mseh <= 0 (PSNR_HVS_LOSSLESS_DB); rgb = the R, G, B mseh
 * added in that order and divided by 3.0f, rgba = the four divided by 4.0f, each with its own psnr. */
typedef struct bu_psnr_hvs_chan {
    double mseh_hvs, mseh_hvsm, psnr_hvs, psnr_hvsm;
} bu_psnr_hvs_chan;
typedef struct bu_psnr_hvs_metrics {
    bu_psnr_hvs_chan y_601_8bit, y_601_float, chan[4], rgb, rgba;
} bu_psnr_hvs_metrics;
/* Returns 0 (and leaves *out alone) on a null pointer or a sums struct whose struct_bytes ends before sum_hvsm does. blocks == 0 gives the 0 / 0 (NaN) of the division. */
BU_HIP_API int bu_psnr_hvs_reduce(const bu_psnr_hvs_sums* sums, bu_psnr_hvs_metrics* out);

/* The 11 x 11 Gaussian of compute_ssim (compute_gaussian_kernel(11, 11, 1.5f * 1.5f, normalize), encoder/basisu_ssim.cpp) in the reference's own order: gauss() with
 * expf / sqrtf of the host's libm, three quadrants copied from the first, the sum a double accumulated x outer and y inner, one_over_sum a double division, every
 * weight float(w * one_over_sum). out[(yd + 5) * 11 + (xd + 5)], yd and xd = -5 .. 5. Returns 0 on a null pointer. */
BU_HIP_API int bu_ssim_gaussian_weights(float out[121]);

#ifdef __cplusplus
}
#endif
#endif
