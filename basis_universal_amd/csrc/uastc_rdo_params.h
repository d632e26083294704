// uastc_rdo_params.h -- the parameters of uastc_rdo as every layer below the C ABI takes them: api_uastc.cpp fills the struct from bu_uastc_rdo_params, the launchers
// of uastc_kernels.h hand it to the kernels as it is, uastc_rdo.h's per-block pieces read it. Plain host and device code.
#pragma once
#include <stdint.h>

namespace bu_uastc {

struct rdo_params {              // uastc_rdo_params, uastc_enc.h:94-134
    float lambda;
    float max_allowed_rms_increase_ratio;
    float skip_block_rms_thresh;
    float max_smooth_block_std_dev;
    float smooth_block_max_error_scale;
    uint32_t lz_dict_size;
    uint32_t lz_literal_cost;
    uint32_t endpoint_refinement;
};

} // namespace bu_uastc
