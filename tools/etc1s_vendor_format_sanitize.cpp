// A stand-alone program around the ETC1S vendor-format conversions (etc1s_vendor_format_targets.h and what it uses of the two headers before it, as g++ compiles
// them), for AddressSanitizer / UndefinedBehaviorSanitizer and for comparing the device's per-block code with the CPU restatement without a GPU:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off -o etc1s_vendor_format_sanitize tools/etc1s_vendor_format_sanitize.cpp
// (tests/test_etc1s_vendor_format_host.py builds and runs it as a child process; nothing of it is loaded into Python).
//   etc1s_vendor_format_sanitize <tables> <image in> <blocks out>
// tables: 76,800 words, the three ATC look-ups 55, 56, 45 and BC1's two (the host statement's, or the device's through bu_hip_etc1s_atc_tables and
// bu_hip_etc1s_bc1_endpoint_tables). image in: words n_endpoints, n_selectors, nbx, nby, has_alpha, then the endpoint palette as the kernels read it, the selector palette,
// nbx * nby endpoint and selector indices and, with has_alpha, as many of the alpha slice (a word each here; an index past its palette is meant to be there, one past
// 65535 is not). Every source block goes through
// vendor_format_block, the function the kernels call, exactly as a lane would, each palette and index array in a heap block of its exact size. blocks out: the ATC
// blocks, the FXT1 blocks ((nbx + 1) / 2 per row), the PVRTC2 RGB blocks, the PVRTC2 RGBA blocks. The few device intrinsics the headers use are stated here for the host.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
struct float2 { float x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{ x, y }; }
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{ x, y, z, w }; }
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
// what etc1s_device.h and etc1s_transcode_kernels.hip give the three headers
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
#include "../basis_universal_amd/csrc/etc1s_bc1.h"
#include "../basis_universal_amd/csrc/etc1s_texture_targets.h"
#include "../basis_universal_amd/csrc/etc1s_block_format_targets.h"
#include "../basis_universal_amd/csrc/etc1s_vendor_format_targets.h"

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

// every source block of the image as a lane would take it; the output in a heap block of its exact size -> the count
template <uint32_t TARGET>
static uint32_t run(const bu::vendor_format_inputs& in, const std::vector<uint16_t>& ei, const std::vector<uint16_t>& si, const uint16_t* aei, const uint16_t* asi, uint32_t nbx, uint32_t nby,
                    std::vector<uint32_t>& out) {
    const size_t blocks = TARGET == bu::VF_FXT1_RGB ? (size_t)((nbx + 1u) / 2u) * nby : (size_t)nbx * nby, words = blocks * (TARGET == bu::VF_FXT1_RGB ? 4u : 2u);
    uint32_t* o = static_cast<uint32_t*>(std::aligned_alloc(16, (words * 4u + 15u) & ~(size_t)15u));
    for (size_t k = 0; k < words; k++) o[k] = 0xA5A5A5A5u;
    uint32_t bad = 0;
    for (uint32_t i = 0; i < nbx * nby; i++) bad += bu::vendor_format_block<TARGET>(in, ei.data(), si.data(), aei, asi, o, i, nbx);
    out.insert(out.end(), o, o + words);
    std::free(o);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <tables> <image in> <blocks out>\n", argv[0]); return 2; }
    std::vector<uint32_t> tables, in;
    if (!read_all(argv[1], tables) || tables.size() != 5u * bu::kAtcEntries || !read_all(argv[2], in) || in.size() < 5) { std::fprintf(stderr, "bad input\n"); return 2; }
    const uint32_t n_ep = in[0], n_sel = in[1], nbx = in[2], nby = in[3], has_alpha = in[4];
    const size_t n = (size_t)nbx * nby, at = 5u + n_ep + n_sel;
    if (!n_ep || !n_sel || !nbx || !nby || has_alpha > 1u || in.size() != at + (has_alpha ? 4u : 2u) * n) { std::fprintf(stderr, "bad image\n"); return 2; }
    const std::vector<uint32_t> ep(in.begin() + 5, in.begin() + 5 + n_ep), sp(in.begin() + 5 + n_ep, in.begin() + at);
    std::vector<uint16_t> ei(n), si(n), aei(has_alpha ? n : 0), asi(has_alpha ? n : 0);
    for (size_t k = at; k < in.size(); k++) {
        if (in[k] > 65535u) { std::fprintf(stderr, "an index does not fit 16 bits\n"); return 2; }
        std::vector<uint16_t>& to = k - at < n ? ei : (k - at < 2u * n ? si : (k - at < 3u * n ? aei : asi));
        to[(k - at) % n] = (uint16_t)in[k];
    }
    const std::vector<uint32_t> atc(tables.begin(), tables.begin() + 3u * bu::kAtcEntries), bc1_5(tables.begin() + 3u * bu::kAtcEntries, tables.begin() + 4u * bu::kAtcEntries),
                                bc1_6(tables.begin() + 4u * bu::kAtcEntries, tables.end());
    const bu::vendor_format_inputs v = { ep.data(), sp.data(), bc1_5.data(), bc1_6.data(), atc.data(), n_ep, n_sel };
    std::vector<uint32_t> out;
    const uint16_t *pa = has_alpha ? aei.data() : nullptr, *ps = has_alpha ? asi.data() : nullptr;
    const uint32_t bad_atc = run<bu::VF_ATC_RGB>(v, ei, si, pa, ps, nbx, nby, out), bad_fxt1 = run<bu::VF_FXT1_RGB>(v, ei, si, pa, ps, nbx, nby, out);
    const uint32_t bad_pvrtc2 = run<bu::VF_PVRTC2_4_RGB>(v, ei, si, pa, ps, nbx, nby, out), bad_pvrtc2a = run<bu::VF_PVRTC2_4_RGBA>(v, ei, si, pa, ps, nbx, nby, out);
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    std::printf("blocks %zu invalid %u %u %u %u\n", n, bad_atc, bad_fxt1, bad_pvrtc2, bad_pvrtc2a);
    return 0;
}
