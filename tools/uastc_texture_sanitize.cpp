// A stand-alone program around the UASTC texture family's core (uastc_transcode.h as g++ compiles it), for AddressSanitizer / UndefinedBehaviorSanitizer:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off -pthread -o uastc_texture_sanitize tools/uastc_texture_sanitize.cpp
// (tests/test_uastc_texture_host.py builds
// and runs it as a child process; nothing of it is loaded into Python): argv[1] random-bit blocks from a fixed generator through every further target of the family
// and both qualities. A hint value that indexed past a table, a shift by a negative amount or a signed overflow would end it with a report and a non-zero status.
// The blocks are dealt to eight threads, each with a stream of its own off the one seed, so the result does not depend on how they are scheduled.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../basis_universal_amd/csrc/uastc_transcode.h"

using namespace bu_uastc;

struct tally { unsigned long long sum = 0; unsigned refused = 0; };

static void run(unsigned stream, unsigned count, tally* out) {
    unsigned long long state = 0x9E3779B97F4A7C15ull * (2ull * stream + 1ull);
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    tally t;
    for (unsigned i = 0; i < count; i++) {
        uint8_t b[16];
        const unsigned long long lo = next(), hi = next();
        std::memcpy(b, &lo, 8); std::memcpy(b + 8, &hi, 8);
        const uint32_t c0 = (uint32_t)(hi >> 61) & 3u, c1 = (uint32_t)(hi >> 59) & 3u;   // the channels move with the block, 3 (the hint's route) among them
        uint64_t w[2] = { 0, 0 };
        if (!transcode_etc<TF_ETC1_RGB, false>(b, 0, 3, w)) { t.refused++; continue; }
        t.sum += w[0];
        transcode_etc<TF_ETC2_RGBA, false>(b, 0, 3, w); t.sum += w[0] ^ w[1];
        transcode_etc<TF_ETC2_EAC_R11, false>(b, c0, c1, w); t.sum += w[0];
        transcode_etc<TF_ETC2_EAC_R11, true>(b, c0, c1, w); t.sum += w[0];
        transcode_etc<TF_ETC2_EAC_RG11, false>(b, c0, c1, w); t.sum += w[0] ^ w[1];
        transcode_etc<TF_ETC2_EAC_RG11, true>(b, c0, c1, w); t.sum += w[0] ^ w[1];
        rgba8 px[16];
        transcode_rgba32(b, px);
        for (int k = 0; k < 16; k++) t.sum += pack_pixel16<TF_RGB565>(px[k]) + pack_pixel16<TF_BGR565>(px[k]) + pack_pixel16<TF_RGBA4444>(px[k]);
    }
    *out = t;
}

int main(int argc, char** argv) {
    const unsigned total = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1000u, streams = 8;
    std::vector<tally> tallies(streams);
    std::vector<std::thread> threads;
    for (unsigned s = 0; s < streams; s++) threads.emplace_back(run, s, total / streams + (s < total % streams ? 1u : 0u), &tallies[s]);
    for (auto& th : threads) th.join();
    tally all;
    for (const tally& t : tallies) { all.sum += t.sum; all.refused += t.refused; }
    std::printf("random %u refused %u sum %llu\n", total, all.refused, all.sum);
    return 0;
}
