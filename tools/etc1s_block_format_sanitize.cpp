// A stand-alone program around the ETC1S block-format conversions (etc1s_block_format_targets.h and, under it, etc1s_texture_targets.h's EAC part, as g++ compiles
// them), for AddressSanitizer / UndefinedBehaviorSanitizer and for comparing the device's per-block code with the CPU restatement without a GPU:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off -o etc1s_block_format_sanitize tools/etc1s_block_format_sanitize.cpp
// (tests/test_etc1s_block_format_host.py builds and runs it as a child process; nothing of it is loaded into Python).
//   etc1s_block_format_sanitize <tables> <blocks in> <blocks out>
// tables: the 30,720 words of the two ASTC look-ups (the host statement's, or the device's through bu_hip_etc1s_astc_tables). blocks in: records of five words
// (colour entry, colour selectors, has alpha, alpha entry, alpha selectors), palette entries as the kernels read them. blocks out: 40 bytes per record, the ASTC
// block, the R11 block, the RG11 block. The few device intrinsics the headers use are stated here for the host.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline
struct uint2 { uint32_t x, y; };
struct float2 { float x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{ x, y }; }
static inline float2 make_float2(float x, float y) { return float2{ x, y }; }
static inline int __ffs(int v) { return __builtin_ffs(v); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
static inline uint32_t __brev(uint32_t v) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(v);
}

#define BU_TAB static const
#include "../basis_universal_amd/csrc/etc1s_transcode_tables.inc"
#include "../basis_universal_amd/csrc/uastc_transcode_tables.inc"
#undef BU_TAB

namespace bu {
// what etc1s_device.h and etc1s_transcode_kernels.hip give the two headers
static const int k_inten_a[8] = { 2, 5, 9, 13, 18, 24, 33, 47 }, k_inten_b[8] = { 8, 17, 29, 42, 60, 80, 106, 183 };
static inline int inten_delta(int table, int sel) { const int v = (sel == 0 || sel == 3) ? k_inten_b[table] : k_inten_a[table]; return sel < 2 ? -v : v; }
static inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
static inline int scale5(int c) { return (c << 3) | (c >> 2); }
struct etc1s_entry { uint32_t r5, g5, b5, table; };
static inline etc1s_entry unpack_entry(uint32_t e) { return etc1s_entry{ e & 31u, (e >> 8) & 31u, (e >> 16) & 31u, (e >> 24) & 7u }; }
static inline uint32_t texel_selector(uint32_t sel, uint32_t x, uint32_t y) { return (sel >> (2u * (y * 4u + x))) & 3u; }
static inline void block_colors(const etc1s_entry& e, uint32_t out[4]) {
    const int r = scale5((int)e.r5), g = scale5((int)e.g5), b = scale5((int)e.b5);
    for (int s = 0; s < 4; s++) {
        const int d = inten_delta((int)e.table, s);
        out[s] = (uint32_t)clamp255(r + d) | ((uint32_t)clamp255(g + d) << 8) | ((uint32_t)clamp255(b + d) << 16);
    }
}
static inline uint32_t pick4(const uint32_t c[4], uint32_t s) { return c[s]; }
}  // namespace bu
#include "../basis_universal_amd/csrc/etc1s_texture_targets.h"
#include "../basis_universal_amd/csrc/etc1s_block_format_targets.h"

template <class T>
static bool read_all(const char* path, std::vector<T>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n / sizeof(T));
    const bool ok = std::fread(out.data(), sizeof(T), out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <tables> <blocks in> <blocks out>\n", argv[0]); return 2; }
    std::vector<uint32_t> tables, in;
    if (!read_all(argv[1], tables) || tables.size() != 2u * bu::kAstcEntries || !read_all(argv[2], in) || in.size() % 5u) { std::fprintf(stderr, "bad input\n"); return 2; }
    std::vector<uint32_t> out;
    out.reserve(in.size() * 2u);
    for (size_t i = 0; i < in.size(); i += 5) {
        const bu::etc1s_entry e = bu::unpack_entry(in[i]), ae = bu::unpack_entry(in[i + 3]);
        const bool has_alpha = in[i + 2] != 0;
        const bu::astc_block b = bu::to_astc(e, in[i + 1], has_alpha, has_alpha ? ae : e, has_alpha ? in[i + 4] : 0u, tables.data());
        const uint2 red = bu::to_eac_r11(e, in[i + 1]), green = has_alpha ? bu::to_eac_r11(ae, in[i + 4]) : bu::opaque_eac_a8();
        const uint32_t words[10] = { (uint32_t)b.lo, (uint32_t)(b.lo >> 32), (uint32_t)b.hi, (uint32_t)(b.hi >> 32), red.x, red.y, red.x, red.y, green.x, green.y };
        out.insert(out.end(), words, words + 10);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    std::printf("blocks %zu\n", in.size() / 5u);
    return 0;
}
