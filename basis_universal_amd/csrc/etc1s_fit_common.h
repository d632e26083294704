// etc1s_fit_common.h -- what the two etc1_optimizer units share (etc1s_block_fit_kernels.hip: one 4x4 block, etc1s_cluster_fit_kernels.hip: all texels of an
// endpoint cluster): the optimizer's two data tables and their upload, the trial colour, the redundant-solution filter, and the launchers' quality -> template argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "etc1s_device.h"
#include "etc1s_kernels.h"
#include "etc1s_tables.inc"

namespace bu {

// The optimizer's two data tables: one copy per including unit, filled by that unit's upload function (upload_fit_tables below) when a context is created.
// (Statically initialised copies were tried: the compiler then addresses them directly instead of through the GOT, which changes every fit kernel.)
__device__ __constant__ static unsigned int c_cluster_fit_order[165];
__device__ __constant__ static unsigned char c_inten_enable_by_spread[256];

// -------------------------------------------------------------------------------------------------------------------
// Shared pieces of etc1_optimizer (etc.cpp:948-1278)
// -------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t perms_for_quality(int quality) {
    return quality == BU_Q_FAST ? 4u : quality == BU_Q_MEDIUM ? 16u : quality == BU_Q_SLOW ? 64u : 165u; // etc.cpp:792-800
}

// m_br/m_bg/m_bb (etc.cpp:1047-1049): round(avg * 31 / 255), float ops in this exact order, no contraction.
__device__ __forceinline__ int avg_to_color5(float avg) {
    const float t = avg * 31.0f;
    const float q = t / 255.0f;
    const float r = q + 0.5f;
    return min(max((int)(uint32_t)r, 0), 31);
}

// One cluster-fit trial colour (etc.cpp:958-986) from the current best solution and selector histogram `hist`.
// Returns false when all three delta sums are zero (the trial is skipped).
__device__ __forceinline__ bool cluster_fit_trial(uint32_t hist, int best_r5, int best_g5, int best_b5, int best_inten,
                                                  float avg_r, float avg_g, float avg_b, int& tr, int& tg, int& tb) {
    const int base_r = scale5(best_r5), base_g = scale5(best_g5), base_b = scale5(best_b5);
    int dr = 0, dg = 0, db = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int cnt = (int)((hist >> (8 * q)) & 255u);
        const int yd = inten_delta(best_inten, q);
        dr += cnt * (clamp255(base_r + yd) - base_r);
        dg += cnt * (clamp255(base_g + yd) - base_g);
        db += cnt * (clamp255(base_b + yd) - base_b);
    }
    if (!(dr | dg | db)) return false;
    const float fr = (float)dr / 8.0f, fg = (float)dg / 8.0f, fb = (float)db / 8.0f;
    {
        const float a = avg_r - fr; const float m = a * 31.0f; const float q = m / 255.0f; const float r = q + 0.5f;
        tr = min(max((int)r, 0), 31);
    }
    {
        const float a = avg_g - fg; const float m = a * 31.0f; const float q = m / 255.0f; const float r = q + 0.5f;
        tg = min(max((int)r, 0), 31);
    }
    {
        const float a = avg_b - fb; const float m = a * 31.0f; const float q = m / 255.0f; const float r = q + 0.5f;
        tb = min(max((int)r, 0), 31);
    }
    return true;
}

// check_for_redundant_solution (etc.cpp:1072-1089) on a 1024-bit filter stored as 32 dwords. Returns true if the colour
// is definitely new (and inserts it). Must be called by exactly one lane per filter, or by lanes that all see the same
// state and write the same value.
__device__ __forceinline__ bool bloom_test_and_set(uint32_t* filter, int r5, int g5, int b5) {
    const uint32_t kh = hash_hsieh3((uint32_t)r5, (uint32_t)g5, (uint32_t)b5);
    const uint32_t h0 = kh & 1023u, h1 = (kh >> 10) & 1023u;
    const uint32_t w0 = filter[h0 >> 5], w1 = filter[h1 >> 5];
    const uint32_t m0 = 1u << (h0 & 31), m1 = 1u << (h1 & 31);
    if ((w0 & m0) && (w1 & m1)) return false;
    if ((h0 >> 5) == (h1 >> 5)) {
        filter[h0 >> 5] = w0 | m0 | m1;
    } else {
        filter[h0 >> 5] = w0 | m0;
        filter[h1 >> 5] = w1 | m1;
    }
    return true;
}

// Host side: the tables of the including unit, on the current device. The same bytes every time, so a repeat (every new context uploads) is harmless.
static inline hipError_t upload_fit_tables() {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_cluster_fit_order), k_cluster_fit_order, sizeof(k_cluster_fit_order));
    if (e != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(c_inten_enable_by_spread), k_inten_enable_by_spread, sizeof(k_inten_enable_by_spread));
}

// f(std::integral_constant<int, Q>{}) for the launcher's quality, Q from LO to BU_Q_UBER. Whatever is not one of the qualities below uber goes to uber, as
// the launchers' if-chains always had it; a launcher that wants another clamp (the cluster fit: fast -> medium) applies it before.
template <int LO, class F>
inline void with_quality(int quality, F&& f) {
    if constexpr (LO <= BU_Q_MEDIUM) {
        if (quality == BU_Q_MEDIUM) { f(std::integral_constant<int, BU_Q_MEDIUM>{}); return; }
    }
    if (quality == BU_Q_SLOW) f(std::integral_constant<int, BU_Q_SLOW>{});
    else f(std::integral_constant<int, BU_Q_UBER>{});
}

} // namespace bu
