// A stand-alone program around the PVRTC1 per-block code (basis_universal_amd/csrc/pvrtc1.h and, for the UASTC routes, the unpacker of uastc_transcode.h, as g++
// compiles them), for AddressSanitizer / UndefinedBehaviorSanitizer and for comparing what the kernels run with the CPU restatement without a GPU:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover -o pvrtc1_sanitize tools/pvrtc1_sanitize.cpp
// (tests/test_pvrtc1_host.py builds and runs it as a child process; nothing of it is loaded into Python). Every file is a sequence of little-endian 32-bit words.
//   pvrtc1_sanitize codes <out>            for v = 0..255: floor and ceil code of 5, 4, 3 bits and of alpha (8 words per v); then the expansions of the 32 + 16 + 8 + 9 codes
//   pvrtc1_sanitize morton <in> <out>      in: records x, y, nbx, nby; out: the block's address
//   pvrtc1_sanitize etc1s <in> <out>       in: nbx, nby, alpha (0 / 1), n_endpoints, n_selectors, the two palettes as the kernels read them, then per block its
//                                          endpoint index, selector index and (alpha) the alpha slice's two; out: nbx * nby blocks of two words, in storage order,
//                                          and one last word: the count of invalid blocks
//   pvrtc1_sanitize uastc <in> <out>       in: nbx, nby, alpha, then nbx * nby blocks of four words; out: the same
// Both image modes run the two passes the way the kernels do: every block's endpoint word first (0 for an invalid block), then per block the nine words around it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../basis_universal_amd/csrc/uastc_transcode.h"
#include "../basis_universal_amd/csrc/pvrtc1.h"

using namespace bu_pvrtc1;

static bool read_all(const char* path, std::vector<uint32_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n / 4u);
    const bool ok = std::fread(out.data(), 4, out.size(), f) == out.size();
    std::fclose(f);
    return ok && n % 4 == 0;
}
static bool write_all(const char* path, const std::vector<uint32_t>& out) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok;
}

// what a block is made of, as pvrtc1_kernels.hip's pvrtc1_block
struct source_block { bool ok; uint32_t entry, sel, alpha_entry, alpha_sel, px[16]; };

template <bool ETC1S, bool ALPHA>
static void image(const std::vector<source_block>& src, uint32_t nbx, uint32_t nby, std::vector<uint32_t>& out) {
    const uint32_t n = nbx * nby;
    std::vector<uint32_t> words(n, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const source_block& b = src[i];
        if (b.ok) words[i] = ETC1S ? etc1s_endpoint_word<ALPHA>(b.entry, b.sel, b.alpha_entry, b.alpha_sel) : pixels_endpoint_word<ALPHA>(b.px);
    }
    out.assign((size_t)n * 2u + 1u, 0u);
    uint32_t invalid = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t x = i & (nbx - 1u), y = i >> log2_pow2(nbx);
        uint32_t around[9];
        for (uint32_t ey = 0; ey < 3; ey++)
            for (uint32_t ex = 0; ex < 3; ex++) around[ey * 3 + ex] = words[(size_t)((y + ey - 1u) & (nby - 1u)) * nbx + ((x + ex - 1u) & (nbx - 1u))];
        const source_block& b = src[i];
        const uint32_t at = morton_address(x, y, nbx, nby);
        if (at >= n) { std::fprintf(stderr, "address %u of block (%u, %u) is past the image\n", at, x, y); std::exit(3); }
        if (!b.ok) { invalid++; continue; }
        int cl[16];
        if (ETC1S) etc1s_texel_values<ALPHA>(b.entry, b.sel, b.alpha_entry, b.alpha_sel, cl);
        else pixels_texel_values<ALPHA>(b.px, cl);
        out[(size_t)at * 2u] = modulation<ALPHA>(around, cl);
        out[(size_t)at * 2u + 1u] = around[4];
    }
    out[(size_t)n * 2u] = invalid;
}

static bool pow2(uint32_t v) { return v && !(v & (v - 1u)); }

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    std::vector<uint32_t> in, out;
    if (!std::strcmp(mode, "codes") && argc == 3) {
        for (uint32_t v = 0; v < 256; v++) {
            const uint32_t row[8] = { floor_code<5>(v), ceil_code<5>(v), floor_code<4>(v), ceil_code<4>(v), floor_code<3>(v), ceil_code<3>(v), floor_alpha(v), ceil_alpha(v) };
            out.insert(out.end(), row, row + 8);
        }
        for (uint32_t c = 0; c < 32; c++) out.push_back(expand<5>(c));
        for (uint32_t c = 0; c < 16; c++) out.push_back(expand<4>(c));
        for (uint32_t c = 0; c < 8; c++) out.push_back(expand<3>(c));
        for (uint32_t c = 0; c < 9; c++) out.push_back(expand_alpha(c));
        return write_all(argv[2], out) ? 0 : 2;
    }
    if (argc != 4 || !read_all(argv[2], in)) { std::fprintf(stderr, "usage: %s codes <out> | morton <in> <out> | etc1s <in> <out> | uastc <in> <out>\n", argv[0]); return 2; }
    if (!std::strcmp(mode, "morton")) {
        if (in.size() % 4u) return 2;
        for (size_t i = 0; i < in.size(); i += 4) {
            if (!pow2(in[i + 2]) || !pow2(in[i + 3]) || in[i] >= in[i + 2] || in[i + 1] >= in[i + 3]) { std::fprintf(stderr, "bad record %zu\n", i / 4); return 2; }
            out.push_back(morton_address(in[i], in[i + 1], in[i + 2], in[i + 3]));
        }
        return write_all(argv[3], out) ? 0 : 2;
    }
    const bool etc1s = !std::strcmp(mode, "etc1s");
    if (!etc1s && std::strcmp(mode, "uastc")) return 2;
    if (in.size() < 3 || !pow2(in[0]) || !pow2(in[1]) || in[2] > 1u) { std::fprintf(stderr, "bad header\n"); return 2; }
    const uint32_t nbx = in[0], nby = in[1], n = nbx * nby;
    const bool alpha = in[2] != 0;
    std::vector<source_block> src(n);
    if (etc1s) {
        if (in.size() < 5) return 2;
        const uint32_t n_ep = in[3], n_sel = in[4], per = alpha ? 4u : 2u;
        if (in.size() != 5u + (size_t)n_ep + n_sel + (size_t)n * per) { std::fprintf(stderr, "bad length\n"); return 2; }
        const uint32_t *ep = in.data() + 5, *sel = ep + n_ep, *idx = sel + n_sel;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t* k = idx + (size_t)i * per;
            source_block& b = src[i];
            b.ok = k[0] < n_ep && k[1] < n_sel && (!alpha || (k[2] < n_ep && k[3] < n_sel));
            if (!b.ok) continue;
            b.entry = ep[k[0]]; b.sel = sel[k[1]];
            b.alpha_entry = alpha ? ep[k[2]] : 0u; b.alpha_sel = alpha ? sel[k[3]] : 0u;
        }
    } else {
        if (in.size() != 3u + (size_t)n * 4u) { std::fprintf(stderr, "bad length\n"); return 2; }
        for (uint32_t i = 0; i < n; i++) {
            uint8_t blk[16];
            std::memcpy(blk, in.data() + 3u + (size_t)i * 4u, 16);
            bu_uastc::rgba8 px[16];
            source_block& b = src[i];
            b.ok = bu_uastc::transcode_rgba32(blk, px);
            if (b.ok) for (int k = 0; k < 16; k++) b.px[k] = bu_uastc::pack_px(px[k].c);
        }
    }
    if (etc1s) { if (alpha) image<true, true>(src, nbx, nby, out); else image<true, false>(src, nbx, nby, out); }
    else { if (alpha) image<false, true>(src, nbx, nby, out); else image<false, false>(src, nbx, nby, out); }
    if (!write_all(argv[3], out)) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::printf("blocks %u invalid %u\n", n, out.back());
    return 0;
}
