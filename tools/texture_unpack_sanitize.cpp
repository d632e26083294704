// A stand-alone program around the texture decode core (basis_universal_amd/csrc/texture_unpack.h as g++ compiles it), for AddressSanitizer /
// UndefinedBehaviorSanitizer on the CPU: random bits into a block decoder are where an out-of-range shift or index hides.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o texture_unpack_sanitize tools/texture_unpack_sanitize.cpp
//   texture_unpack_sanitize [blocks per format, default 2000000]
// Per format that many random-bit blocks from one fixed xorshift stream go through the block function, each from a heap buffer of exactly the block's size into
// one of exactly 64 bytes. Raw random bits rarely pass ASTC's header checks, so three of four ASTC blocks get a block mode of the 4x4 footprint forced in (grid 4
// wide, or 2 / 3 wide) and the rest stay raw. PVRTC1 runs as whole images of 1x1, 2x1, 1x2, 2x2, 8x2 and 4x8 blocks, every block of each. Prints per format the
// blocks, how many were refused and a digest of the texels; nothing of it is loaded into Python, and it is never run on a GPU machine.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../basis_universal_amd/csrc/texture_unpack.h"

using namespace bu_unpack;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_bits() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

template <uint32_t FORMAT>
static void run(const char* name, uint32_t count) {
    const uint32_t unit = texture_bytes_per_block(FORMAT);
    uint8_t* in = (uint8_t*)std::malloc(unit);
    uint8_t* out = (uint8_t*)std::malloc(64);
    uint64_t digest = 1469598103934665603ull;
    uint32_t refused = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t w[2] = { next_bits(), next_bits() };
        if (FORMAT == UF_ASTC_4x4 && (i & 3u)) {
            if (i & 1u) w[0] &= ~0x18Cull;                 // bits 2, 3, 7, 8 clear: a grid 4 wide
            else w[0] = (w[0] | 0x10Cull);                 // bits 2, 3, 8 set: a grid 2 or 3 wide
            if ((w[0] & 3u) == 0u) w[0] |= 1u + (i & 2u);  // and not the layouts of the wider footprints
        }
        std::memcpy(in, w, unit);
        if (!unpack_texture_block<FORMAT>(in, out)) refused++;
        for (uint32_t k = 0; k < 64; k++) digest = (digest ^ out[k]) * 1099511628211ull;
    }
    std::free(in);
    std::free(out);
    std::printf("%-8s blocks %u refused %u digest %016llx\n", name, count, refused, (unsigned long long)digest);
}

static void run_pvrtc1(uint32_t count) {
    static const uint32_t sizes[6][2] = { { 1, 1 }, { 2, 1 }, { 1, 2 }, { 2, 2 }, { 8, 2 }, { 4, 8 } };
    uint64_t digest = 1469598103934665603ull;
    uint32_t done = 0;
    uint8_t* out = (uint8_t*)std::malloc(64);
    for (uint32_t round = 0; done < count; round++) {
        const uint32_t nbx = sizes[round % 6u][0], nby = sizes[round % 6u][1], n = nbx * nby;
        uint8_t* blocks = (uint8_t*)std::malloc((size_t)n * 8u);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t w = next_bits();
            std::memcpy(blocks + (size_t)i * 8u, &w, 8);
        }
        for (uint32_t by = 0; by < nby; by++)
            for (uint32_t bx = 0; bx < nbx; bx++) {
                unpack_pvrtc1_block(blocks, nbx, nby, bx, by, out);
                for (uint32_t k = 0; k < 64; k++) digest = (digest ^ out[k]) * 1099511628211ull;
            }
        std::free(blocks);
        done += n;
    }
    std::free(out);
    std::printf("%-8s blocks %u refused 0 digest %016llx\n", "pvrtc1", done, (unsigned long long)digest);
}

int main(int argc, char** argv) {
    const uint32_t count = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 2000000u;
    run<UF_ETC1>("etc1", count);
    run<UF_ETC2_RGBA>("etc2", count);
    run<UF_EAC_R11>("r11", count);
    run<UF_EAC_RG11>("rg11", count);
    run<UF_ASTC_4x4>("astc", count);
    run<UF_BC1>("bc1", count);
    run<UF_BC3>("bc3", count);
    run<UF_BC4>("bc4", count);
    run<UF_BC5>("bc5", count);
    run<UF_BC7>("bc7", count);
    run_pvrtc1(count);
    return 0;
}
