// ssim_reduce.h -- avg_image's running binary32 sum (ssim.h) in the form the device evaluates it (fsum_scan.h), shared by ssim_kernels.hip and, compiled with g++, by the
// CPU tests (tests/native/ssim_host.cpp): chunks of consecutive addends, for each a guess of the binade the running state is in
// when the chunk starts, and the chunk's stretch for that binade and for the one above. The ordered walk applies a stretch where it is valid for the real state and
// otherwise adds the chunk's addends one by one -- which is always right, so the result is the serial sum's whatever the guess was.
#pragma once
#include "fsum_scan.h"
#include "ssim.h"

namespace bu {

BU_SSIM_HD uint32_t ssim_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
BU_SSIM_HD float ssim_float(uint32_t u) { return __builtin_bit_cast(float, u); }

struct ssim_chunk { int32_t E; uint32_t neg; fsum::stretch s[2]; };   // s[c]: for a state of sign `neg` with biased exponent E + c

// prefix: any approximation of the sum of everything before the chunk. The guess leaves 2^-10 of room below it: the float chain drifts from the exact sum by a few
// ulps per thousand addends at the most, and a state just above a power of two would otherwise be guessed one binade too high about half of the time.
BU_SSIM_HD ssim_chunk ssim_chunk_build(const float* v, uint32_t n, double prefix) {
    ssim_chunk m;
    m.neg = prefix < 0 ? 1u : 0u;
    const double mag = (prefix < 0 ? -prefix : prefix) * (1.0 - 0.0009765625);
    m.E = fsum::state_exp(ssim_bits((float)mag));
    BU_SSIM_UNROLL
    for (int c = 0; c < 2; c++) {
        fsum::stretch s = fsum::identity();
        bool bad = false;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t a = ssim_bits(v[i]);
            if ((a << 1) == 0) continue;
            fsum::push_fast(s, fsum::decode_fast(fsum::split(a, m.neg != 0), m.E + c, bad));
        }
        if (bad || m.E + c < 1 || m.E + c > 253) fsum::poison(s);
        m.s[c] = s;
    }
    return m;
}

// state (float bits) before the chunk -> after it; *walked is raised where the addends had to be added one by one
BU_SSIM_HD uint32_t ssim_chunk_walk(uint32_t state, const ssim_chunk& m, const float* v, uint32_t n, uint32_t* walked) {
    const int c = fsum::state_exp(state) - m.E;
    if (fsum::state_ok(state) && ((state >> 31) != 0) == (m.neg != 0) && (c == 0 || c == 1)) {
        const fsum::stretch& s = c ? m.s[1] : m.s[0];
        if (fsum::applies(s, fsum::state_k(state))) return fsum::apply(s, state);
    }
    float f = ssim_float(state);
    for (uint32_t i = 0; i < n; i++) f = f + v[i];
    ++*walked;
    return ssim_bits(f);
}

}  // namespace bu
