// etc1s_decode.cpp -- see etc1s_decode.h. Written from the formats as etc1s_backend.cpp / entropy.h write them; the reference's reader
// (transcoder/basisu_transcoder.cpp:8257-8841, basisu_transcoder_internal.h:293-751) is what a stream means where the two could differ.
//
// Safety: the file is untrusted. Every section is located through checked (offset, length) pairs (`span`), the bit reader never reads past its section (it
// supplies zero bits there and remembers that it had to; a decode that consumed such bits is an error), every table is checked to be a complete prefix code before
// it is used, every decoded index is checked against its palette before it is stored, and every count that sizes an allocation is bounded before it is used.
#include "etc1s_decode.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <thread>

#include "../../../include/basisu_hip_etc1s_decode.h"
#include "entropy.h"

namespace bu {
namespace {

enum : uint32_t {  // transcoder/basisu_transcoder_internal.h:256-267, the same values etc1s_backend.cpp codes with
    kEndpointPredSymbols = 4 * 4 * 4 * 4 + 1, kEndpointPredRepeatLast = kEndpointPredSymbols - 1, kEndpointPredMinRepeat = 3, kEndpointPredCountVlcBits = 4,
    kNoEndpointPred = 3, kSelectorRleThresh = 3, kSelectorRleCountTotal = 64,
    kMaxPaletteEntries = 65535,         // the containers' counts are 16 bits wide, and so are the index arrays
    kMaxDimension = 16384, kMaxTotalBlocks = 1u << 28, kMaxDecodeThreads = 16
};

std::string fmt(const char* f, ...) {
    char buf[320];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// ---------------------------------------------------------------- checked views of the file
struct span {
    const uint8_t* p = nullptr;
    uint64_t n = 0;
};

struct file_view {
    const uint8_t* data;
    uint64_t size;
    std::string* error;
    bool need(uint64_t ofs, uint64_t len, const char* what) const {
        if (ofs > size || len > size - ofs) {
            *error = fmt("truncated or corrupt file: %s needs bytes %llu..%llu of %llu", what, (unsigned long long)ofs, (unsigned long long)(ofs + len), (unsigned long long)size);
            return false;
        }
        return true;
    }
    uint64_t le(uint64_t ofs, int bytes) const {  // caller has checked the range
        uint64_t v = 0;
        for (int i = 0; i < bytes; i++) v |= (uint64_t)data[ofs + i] << (8 * i);
        return v;
    }
};

// ---------------------------------------------------------------- bits and prefix codes
class bit_reader {  // LSB first, like bit_writer
public:
    explicit bit_reader(span s) : m_p(s.p), m_end(s.p + s.n), m_avail(s.n * 8) {}
    uint32_t peek(uint32_t n) {  // n <= 25
        while (m_fill < n) { m_acc |= (uint64_t)(m_p < m_end ? *m_p++ : 0) << m_fill; m_fill += 8; }
        return (uint32_t)(m_acc & ((1ull << n) - 1ull));
    }
    void drop(uint32_t n) { m_acc >>= n; m_fill -= n; m_used += n; }
    uint32_t get(uint32_t n) { if (!n) return 0; const uint32_t v = peek(n); drop(n); return v; }
    bool get_vlc(uint32_t chunk_bits, uint32_t& out) {  // bit_writer::put_vlc; false: more chunks than a 32-bit value has
        uint32_t v = 0, shift = 0;
        for (;;) {
            const uint32_t c = get(chunk_bits + 1);
            if (shift >= 32) return false;
            v |= (c & ((1u << chunk_bits) - 1u)) << shift;
            if (!(c >> chunk_bits)) break;
            shift += chunk_bits;
        }
        out = v;
        return true;
    }
    bool overrun() const { return m_used > m_avail; }  // consumed bits the section does not hold

private:
    const uint8_t* m_p;
    const uint8_t* m_end;
    uint64_t m_avail, m_used = 0, m_acc = 0;
    uint32_t m_fill = 0;
};

class huffman_decoder {
public:
    // sizes[n]: code length per symbol, 0 = unused. The codes are the canonical ones of huffman_table::init. A table has to be a complete prefix code
    // (Kraft sum exactly one) or hold a single 1-bit code, which is what the writer makes of a one-symbol histogram.
    bool init(const uint8_t* sizes, uint32_t n, std::string& why) {
        m_syms.clear();
        uint32_t count[kHuffMaxCodeSize + 1] = {0};
        for (uint32_t i = 0; i < n; i++) {
            if (sizes[i] > kHuffMaxCodeSize) { why = fmt("a code of %u bits is longer than the limit of %u", sizes[i], kHuffMaxCodeSize); return false; }
            count[sizes[i]]++;
        }
        count[0] = 0;
        uint32_t used = 0;
        uint64_t kraft = 0;
        for (uint32_t l = 1; l <= kHuffMaxCodeSize; l++) { used += count[l]; kraft += (uint64_t)count[l] << (kHuffMaxCodeSize - l); }
        if (!used) { why = "no symbol has a code"; return false; }
        if (kraft != (1ull << kHuffMaxCodeSize) && !(used == 1 && count[1] == 1)) {
            why = kraft > (1ull << kHuffMaxCodeSize) ? "the code lengths describe more codes than fit (a code would have to be longer than its stated length)"
                                                      : "the code lengths leave part of the code space unused";
            return false;
        }
        uint32_t code = 0, at = 0;
        for (uint32_t l = 1; l <= kHuffMaxCodeSize; l++) {
            code = (code + count[l - 1]) << 1;
            m_first[l] = code; m_offset[l] = at; m_count[l] = count[l];
            at += count[l];
        }
        m_syms.resize(used);
        uint32_t next[kHuffMaxCodeSize + 1];
        for (uint32_t l = 1; l <= kHuffMaxCodeSize; l++) next[l] = m_offset[l];
        for (uint32_t s = 0; s < n; s++) if (sizes[s]) m_syms[next[sizes[s]]++] = (uint16_t)s;
        // codes of up to kFastBits bits: (length << 16 | symbol) at every index whose low bits are the code, bit-reversed as it travels
        m_fast.assign(1u << kFastBits, 0);
        for (uint32_t l = 1; l <= kFastBits; l++)
            for (uint32_t k = 0; k < m_count[l]; k++) {
                uint32_t c = m_first[l] + k, rev = 0;
                for (uint32_t b = 0; b < l; b++, c >>= 1) rev = (rev << 1) | (c & 1u);
                for (uint32_t i = rev; i < (1u << kFastBits); i += 1u << l) m_fast[i] = (l << 16) | m_syms[m_offset[l] + k];
            }
        if (used == 1) m_fast.assign(1u << kFastBits, (1u << 16) | m_syms[0]);   // the single 1-bit code: either bit pattern is that symbol
        return true;
    }
    bool valid() const { return !m_syms.empty(); }
    uint32_t decode(bit_reader& r) const {  // a complete code always resolves
        const uint32_t e = m_fast[r.peek(kFastBits)];
        if (e) { r.drop(e >> 16); return e & 0xFFFFu; }
        uint32_t code = 0;
        for (uint32_t l = 1; l <= kHuffMaxCodeSize; l++) {
            code = (code << 1) | r.get(1);
            if (code - m_first[l] < m_count[l] && code >= m_first[l]) return m_syms[m_offset[l] + (code - m_first[l])];
        }
        return m_syms[0];  // not reached: init() admits complete codes only
    }

private:
    enum : uint32_t { kFastBits = 10 };
    std::vector<uint16_t> m_syms;  // symbols sorted by (length, symbol)
    std::vector<uint32_t> m_fast;
    uint32_t m_first[kHuffMaxCodeSize + 1] = {0}, m_offset[kHuffMaxCodeSize + 1] = {0}, m_count[kHuffMaxCodeSize + 1] = {0};
};

// bit_writer::put_table read back (= bitwise_decoder::read_huffman_table). An empty table (no symbols used) is legal here and left invalid: who needs it says so.
bool read_table(bit_reader& r, huffman_decoder& t, const char* name, std::string& error) {
    const uint32_t used = r.get(kHuffMaxSymsLog2);
    if (!used) return true;
    const uint32_t sent = r.get(5);
    if (sent < 1 || sent > kHuffCodelengthCodes) { error = fmt("Huffman table '%s': %u code-length codes where 1..%u are possible", name, sent, kHuffCodelengthCodes); return false; }
    static const uint8_t order[kHuffCodelengthCodes] = {17, 18, 19, 20, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 16};
    uint8_t cl_sizes[kHuffCodelengthCodes] = {0};
    for (uint32_t i = 0; i < sent; i++) cl_sizes[order[i]] = (uint8_t)r.get(3);
    huffman_decoder cl;
    std::string why;
    if (!cl.init(cl_sizes, kHuffCodelengthCodes, why)) { error = fmt("Huffman table '%s': its code-length code is invalid: %s", name, why.c_str()); return false; }
    std::vector<uint8_t> sizes(used, 0);
    uint32_t cur = 0;
    while (cur < used) {
        if (r.overrun()) { error = fmt("Huffman table '%s': truncated", name); return false; }
        const uint32_t c = cl.decode(r);
        if (c <= 16) sizes[cur++] = (uint8_t)c;
        else if (c == kHuffSmallZeroRun) cur += r.get(3) + 3;
        else if (c == kHuffBigZeroRun) cur += r.get(7) + 11;
        else {
            const uint32_t run = c == kHuffSmallRepeat ? r.get(2) + 3 : r.get(7) + 7;
            if (!cur || !sizes[cur - 1]) { error = fmt("Huffman table '%s': a repeat with no code length before it", name); return false; }
            if (run > used - cur) { error = fmt("Huffman table '%s': a repeat runs past its %u symbols", name, used); return false; }
            for (uint32_t k = 0; k < run; k++, cur++) sizes[cur] = sizes[cur - 1];
        }
    }
    if (cur != used) { error = fmt("Huffman table '%s': a zero run runs past its %u symbols", name, used); return false; }
    if (r.overrun()) { error = fmt("Huffman table '%s': truncated", name); return false; }
    if (!t.init(sizes.data(), used, why)) { error = fmt("Huffman table '%s': %s", name, why.c_str()); return false; }
    return true;
}

// ---------------------------------------------------------------- palettes and slice models
bool decode_endpoint_palette(span s, uint32_t n, std::vector<uint8_t>& out, std::string& error) {
    bit_reader r(s);
    huffman_decoder m[3], mi;
    if (!read_table(r, m[0], "endpoint colour delta 0", error) || !read_table(r, m[1], "endpoint colour delta 1", error) || !read_table(r, m[2], "endpoint colour delta 2", error) ||
        !read_table(r, mi, "endpoint intensity delta", error)) return false;
    if (!m[0].valid() || !m[1].valid() || !m[2].valid() || !mi.valid()) { error = "endpoint palette: an empty Huffman table"; return false; }
    const bool gray = r.get(1) != 0;
    out.assign((size_t)n * 4, 0);
    uint32_t prev[3] = {16, 16, 16}, prev_inten = 0;
    for (uint32_t i = 0; i < n; i++) {
        prev_inten = (mi.decode(r) + prev_inten) & 7u;
        out[i * 4 + 3] = (uint8_t)prev_inten;
        for (uint32_t c = 0; c < (gray ? 1u : 3u); c++) {
            const huffman_decoder& t = prev[c] <= 9 ? m[0] : (prev[c] <= 21 ? m[1] : m[2]);  // COLOR5_PAL0/1_PREV_HI
            prev[c] = (prev[c] + t.decode(r)) & 31u;
            out[i * 4 + c] = (uint8_t)prev[c];
        }
        if (gray) out[i * 4 + 1] = out[i * 4 + 2] = out[i * 4];
        if (r.overrun()) { error = fmt("truncated or corrupt file: the endpoint palette ends inside entry %u of %u", i, n); return false; }
    }
    return true;
}

bool decode_selector_palette(span s, uint32_t n, std::vector<uint32_t>& out, std::string& error) {
    bit_reader r(s);
    if (r.get(1)) { error = "the selector palette uses a global codebook, which is not supported"; return false; }
    if (r.get(1)) { error = "the selector palette uses a hybrid global codebook, which is not supported"; return false; }
    const bool raw = r.get(1) != 0;
    out.assign(n, 0);
    huffman_decoder model;
    if (!raw) {
        if (!read_table(r, model, "selector palette delta", error)) return false;
        if (n > 1 && !model.valid()) { error = "selector palette: an empty Huffman table"; return false; }
    }
    uint32_t prev = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t cur = 0;
        for (uint32_t j = 0; j < 4; j++) cur |= ((raw || !i) ? r.get(8) : (model.decode(r) & 255u)) << (8 * j);
        if (!raw && i) cur ^= prev;
        out[i] = prev = cur;
        if (r.overrun()) { error = fmt("truncated or corrupt file: the selector palette ends inside entry %u of %u", i, n); return false; }
    }
    return true;
}

struct slice_models {
    huffman_decoder pred, delta, selector, rle;
    uint32_t history_size = 0;
};

bool decode_tables(span s, slice_models& m, std::string& error) {
    bit_reader r(s);
    if (!read_table(r, m.pred, "endpoint predictor", error) || !read_table(r, m.delta, "endpoint delta", error) || !read_table(r, m.selector, "selector", error) ||
        !read_table(r, m.rle, "selector history run", error)) return false;
    if (!m.pred.valid() || !m.delta.valid() || !m.selector.valid() || !m.rle.valid()) { error = "slice tables: an empty Huffman table"; return false; }
    m.history_size = r.get(13);
    if (r.overrun()) { error = "truncated or corrupt file: the slice tables end early"; return false; }
    if (!m.history_size) { error = "slice tables: a selector history buffer of size 0"; return false; }
    return true;
}

// ---------------------------------------------------------------- one slice
struct slice_job {
    span bits;
    uint32_t nbx = 0, nby = 0, image = 0;
    bool alpha = false;
    uint64_t first_block = 0;
    std::string error;
};

bool decode_slice(slice_job& job, const slice_models& m, uint32_t n_endpoints, uint32_t n_selectors, uint16_t* endpoint_out, uint16_t* selector_out) {
    const uint32_t nbx = job.nbx, nby = job.nby;
    const uint64_t total = (uint64_t)nbx * nby;
    auto fail = [&](uint32_t bx, uint32_t by, const std::string& what) {
        job.error = fmt("image %u %s slice, block (%u, %u): %s", job.image, job.alpha ? "alpha" : "colour", bx, by, what.c_str());
        return false;
    };
    bit_reader r(job.bits);
    // approx_move_to_front (transcoder_internal.h:863-925): starts as zeros, new values enter at a rover in the upper half, a used one swaps towards the front
    std::vector<uint32_t> history(m.history_size, 0);
    uint32_t rover = m.history_size / 2;
    const uint32_t rle_sym = n_selectors + m.history_size;
    std::vector<uint8_t> row_pred_bits((nbx + 1) / 2 * 2 + 2, 0);   // the odd row's half of each macroblock's predictor symbol
    uint32_t cur_pred_bits = 0, prev_pred_sym = 0, pred_repeat = 0, prev_endpoint = 0, selector_rle = 0;
    for (uint32_t by = 0; by < nby; by++) {
        uint16_t* ep_row = endpoint_out + (size_t)by * nbx;
        const uint16_t* ep_up = by ? ep_row - nbx : ep_row;   // read only when by > 0
        for (uint32_t bx = 0; bx < nbx; bx++) {
            if (!(bx & 1)) {
                if (!(by & 1)) {
                    if (pred_repeat) {
                        pred_repeat--;
                        cur_pred_bits = prev_pred_sym;
                    } else {
                        cur_pred_bits = m.pred.decode(r);
                        if (cur_pred_bits >= kEndpointPredSymbols) return fail(bx, by, "an endpoint predictor symbol out of range");
                        if (cur_pred_bits == kEndpointPredRepeatLast) {
                            uint32_t v;
                            if (!r.get_vlc(kEndpointPredCountVlcBits, v) || v > total) return fail(bx, by, "an endpoint predictor run longer than the slice");
                            pred_repeat = v + kEndpointPredMinRepeat - 1;
                            cur_pred_bits = prev_pred_sym;
                        } else {
                            prev_pred_sym = cur_pred_bits;
                        }
                    }
                    row_pred_bits[bx] = (uint8_t)(cur_pred_bits >> 4);
                } else {
                    cur_pred_bits = row_pred_bits[bx];
                }
            }
            const uint32_t pred = cur_pred_bits & 3u;
            cur_pred_bits >>= 2;
            uint32_t endpoint;
            if (pred == 0) {
                if (!bx) return fail(bx, by, "endpoint predicted from the left neighbour in the first column");
                endpoint = prev_endpoint;
            } else if (pred == 1) {
                if (!by) return fail(bx, by, "endpoint predicted from the upper neighbour in the first row");
                endpoint = ep_up[bx];
            } else if (pred == 2) {
                if (!bx || !by) return fail(bx, by, "endpoint predicted from the upper-left neighbour in the first row or column");
                endpoint = ep_up[bx - 1];
            } else {
                endpoint = m.delta.decode(r) + prev_endpoint;
                if (endpoint >= n_endpoints) endpoint -= n_endpoints;
            }
            if (endpoint >= n_endpoints) return fail(bx, by, fmt("endpoint index %u is past the palette of %u entries", endpoint, n_endpoints));
            ep_row[bx] = (uint16_t)endpoint;
            prev_endpoint = endpoint;

            uint32_t sym;
            if (selector_rle) {
                selector_rle--;
                sym = n_selectors;
            } else {
                sym = m.selector.decode(r);
                if (sym == rle_sym) {
                    const uint32_t run = m.rle.decode(r);
                    uint32_t count;
                    if (run >= kSelectorRleCountTotal) return fail(bx, by, "a selector run symbol out of range");
                    if (run == kSelectorRleCountTotal - 1) {
                        uint32_t v;
                        if (!r.get_vlc(7, v) || v > total) return fail(bx, by, "a selector run longer than the slice");
                        count = v + kSelectorRleThresh;
                    } else {
                        count = run + kSelectorRleThresh;
                    }
                    if (count > total) return fail(bx, by, "a selector run longer than the slice");
                    selector_rle = count - 1;
                    sym = n_selectors;
                }
            }
            uint32_t selector;
            if (sym >= n_selectors) {
                const uint32_t h = sym - n_selectors;
                if (h >= m.history_size) return fail(bx, by, fmt("selector symbol %u is past the palette of %u entries and the history of %u", sym, n_selectors, m.history_size));
                selector = history[h];
                if (h) std::swap(history[h / 2], history[h]);
            } else {
                selector = sym;
                history[rover++] = selector;
                if (rover == m.history_size) rover = m.history_size / 2;
            }
            if (selector >= n_selectors) return fail(bx, by, fmt("selector index %u is past the palette of %u entries", selector, n_selectors));
            selector_out[(size_t)by * nbx + bx] = (uint16_t)selector;
        }
        if (r.overrun()) return fail(0, by, "truncated or corrupt file: the slice's data ends before its last block");
    }
    return true;
}

// ---------------------------------------------------------------- containers
struct sections {
    span endpoints, selectors, tables;
};

bool finish_image_list(etc1s_file& f, std::string& error) {
    std::sort(f.images.begin(), f.images.end(), [](const etc1s_image& a, const etc1s_image& b) {
        return a.level != b.level ? a.level < b.level : (a.layer != b.layer ? a.layer < b.layer : a.face < b.face);
    });
    for (size_t i = 1; i < f.images.size(); i++)
        if (f.images[i].level == f.images[i - 1].level && f.images[i].layer == f.images[i - 1].layer && f.images[i].face == f.images[i - 1].face) {
            error = fmt("two colour slices for level %u, layer %u, face %u", f.images[i].level, f.images[i].layer, f.images[i].face);
            return false;
        }
    uint64_t at = 0;
    for (etc1s_image& im : f.images) {
        const uint64_t n = (uint64_t)im.num_blocks_x * im.num_blocks_y;
        im.first_block = at; at += n;
        if (im.alpha_len) { im.alpha_first_block = at; at += n; f.has_alpha_slices = true; }
    }
    f.total_blocks = at;
    return true;
}

bool parse_basis(const file_view& v, etc1s_file& f, sections& sec) {
    const uint32_t kHeader = 77, kSlice = 23;   // sizeof(basis_file_header), sizeof(basis_slice_desc) (transcoder/basisu_file_headers.h)
    std::string& error = *v.error;
    if (!v.need(0, kHeader, "the .basis header")) return false;
    const uint32_t ver = (uint32_t)v.le(2, 2), hsize = (uint32_t)v.le(4, 2), total_slices = (uint32_t)v.le(14, 3), total_images = (uint32_t)v.le(17, 3);
    const uint32_t tex_format = v.data[20], flags = (uint32_t)v.le(21, 2), tex_type = v.data[23];
    if (ver != 0x13 || hsize != kHeader) { error = fmt("unsupported .basis version %#x / header size %u", ver, hsize); return false; }
    if (tex_format != 0 || !(flags & 1u)) {
        error = fmt("not an ETC1S file: the .basis texture format is %u (%s)", tex_format, tex_format == 1 ? "UASTC LDR 4x4: read_uastc_file / transcode_file read those" : "not ETC1S");
        return false;
    }
    if (tex_type == 3) { error = "video files are not supported: a P-frame's blocks may repeat the previous frame's indices, which this reader does not keep"; return false; }
    if (tex_type > 4) { error = fmt("unknown .basis texture type %u", tex_type); return false; }
    if (v.le(8, 4) + kHeader > v.size) {
        error = fmt("truncated or corrupt file: the .basis header promises %llu bytes, %llu are here", (unsigned long long)(v.le(8, 4) + kHeader), (unsigned long long)v.size);
        return false;
    }
    f.container = 0; f.tex_type = tex_type; f.srgb = (flags & 16u) != 0;
    f.num_endpoints = (uint32_t)v.le(39, 2); f.num_selectors = (uint32_t)v.le(48, 2);
    const uint64_t ep_ofs = v.le(41, 4), ep_len = v.le(45, 3), sel_ofs = v.le(50, 4), sel_len = v.le(54, 3), tab_ofs = v.le(57, 4), tab_len = v.le(61, 4), descs_ofs = v.le(65, 4);
    if (!total_slices || !total_images) { error = "a .basis file without slices"; return false; }
    if (!v.need(descs_ofs, (uint64_t)kSlice * total_slices, "the slice descriptors") || !v.need(ep_ofs, ep_len, "the endpoint palette") ||
        !v.need(sel_ofs, sel_len, "the selector palette") || !v.need(tab_ofs, tab_len, "the slice tables")) return false;
    sec.endpoints = span{v.data + ep_ofs, ep_len}; sec.selectors = span{v.data + sel_ofs, sel_len}; sec.tables = span{v.data + tab_ofs, tab_len};
    f.faces = tex_type == 2 ? 6 : 1;
    if (total_images % f.faces) { error = "a cubemap .basis file whose image count is not a multiple of 6"; return false; }
    f.layers = total_images / f.faces;
    // a colour slice opens an image level; with the alpha flag set its alpha slice follows it directly (basis_file.cpp:125-160)
    const bool alpha_pairs = (flags & 4u) != 0;
    uint32_t levels = 0;
    for (uint32_t i = 0; i < total_slices; i++) {
        const uint64_t at = descs_ofs + (uint64_t)kSlice * i;
        const uint32_t image = (uint32_t)v.le(at, 3), level = v.data[at + 3], sflags = v.data[at + 4];
        const uint32_t ow = (uint32_t)v.le(at + 5, 2), oh = (uint32_t)v.le(at + 7, 2), nbx = (uint32_t)v.le(at + 9, 2), nby = (uint32_t)v.le(at + 11, 2);
        const uint64_t ofs = v.le(at + 13, 4), len = v.le(at + 17, 4);
        if (image >= total_images || level >= 16 || !ow || !oh || nbx != (ow + 3) / 4 || nby != (oh + 3) / 4) { error = fmt("slice %u: inconsistent descriptor", i); return false; }
        if (!v.need(ofs, len, fmt("slice %u", i).c_str())) return false;
        if (sflags & 1u) {
            if (!alpha_pairs || f.images.empty()) { error = fmt("slice %u: an alpha slice without a colour slice before it", i); return false; }
            etc1s_image& im = f.images.back();
            if (im.alpha_len || im.layer * f.faces + im.face != image || im.level != level || im.num_blocks_x != nbx || im.num_blocks_y != nby || !len) {
                error = fmt("slice %u: an alpha slice that does not match the colour slice before it", i);
                return false;
            }
            im.alpha_ofs = ofs; im.alpha_len = len;
        } else {
            if (alpha_pairs && !f.images.empty() && !f.images.back().alpha_len) { error = fmt("slice %u: the colour slice before it has no alpha slice", i); return false; }
            etc1s_image im;
            im.level = level; im.layer = image / f.faces; im.face = image % f.faces;
            im.width = ow; im.height = oh; im.num_blocks_x = nbx; im.num_blocks_y = nby; im.rgb_ofs = ofs; im.rgb_len = len;
            f.images.push_back(im);
            levels = std::max(levels, level + 1);
        }
    }
    if (f.images.empty()) { error = "a .basis file without colour slices"; return false; }
    if (alpha_pairs && !f.images.back().alpha_len) { error = "the last colour slice has no alpha slice"; return false; }
    f.levels = levels;
    if (!finish_image_list(f, error)) return false;
    f.width = f.images[0].width; f.height = f.images[0].height;
    return true;
}

bool ktx2_is_video(const file_view& v, uint64_t kvd_ofs, uint64_t kvd_len) {  // the key the reference's writer marks video with (comp.cpp: "KTXanimData")
    static const char key[] = "KTXanimData";
    uint64_t at = kvd_ofs;
    const uint64_t end = kvd_ofs + kvd_len;
    while (end - at >= 4) {
        const uint64_t len = v.le(at, 4);
        at += 4;
        if (len > end - at) return false;
        if (len >= sizeof(key) && !std::memcmp(v.data + at, key, sizeof(key))) return true;
        at += (len + 3) & ~3ull;
        if (at > end) return false;
    }
    return false;
}

bool parse_ktx2(const file_view& v, etc1s_file& f, sections& sec) {
    std::string& error = *v.error;
    if (!v.need(0, 80, "the KTX2 header")) return false;
    const uint32_t vk_format = (uint32_t)v.le(12, 4), width = (uint32_t)v.le(20, 4), height = (uint32_t)v.le(24, 4), depth = (uint32_t)v.le(28, 4), layers = (uint32_t)v.le(32, 4),
                   faces = (uint32_t)v.le(36, 4), levels = (uint32_t)v.le(40, 4), scheme = (uint32_t)v.le(44, 4);
    const uint64_t dfd_ofs = v.le(48, 4), dfd_len = v.le(52, 4), kvd_ofs = v.le(56, 4), kvd_len = v.le(60, 4), sgd_ofs = v.le(64, 8), sgd_len = v.le(72, 8);
    if (vk_format != 0 || depth || !width || !height || width > kMaxDimension || height > kMaxDimension || (faces != 1 && faces != 6) || levels < 1 || levels > 16) {
        error = "not a 2D Basis Universal KTX2 file";
        return false;
    }
    if (!v.need(80, 24ull * levels, "the level index") || !v.need(dfd_ofs, dfd_len, "the data format descriptor") || !v.need(kvd_ofs, kvd_len, "the key-value data")) return false;
    const uint32_t model = dfd_len >= 44 ? v.data[dfd_ofs + 12] : 0;
    if (scheme != 1 || model != 163) {
        if (model == 166) error = "not an ETC1S file: the KTX2 data format descriptor is UASTC LDR 4x4's (colour model 166): read_uastc_file / transcode_file read those";
        else error = fmt("not an ETC1S file: KTX2 supercompression scheme %u and colour model %u where BasisLZ (1) and ETC1S (163) are expected", scheme, model);
        return false;
    }
    if (ktx2_is_video(v, kvd_ofs, kvd_len)) { error = "video files are not supported: a P-frame's blocks may repeat the previous frame's indices, which this reader does not keep"; return false; }
    const uint64_t n_layers = std::max(layers, 1u), per_level = n_layers * faces;
    if (n_layers > 0xFFFFFFull) { error = "not a 2D Basis Universal KTX2 file"; return false; }
    const uint64_t n_images = per_level * levels;
    if (!v.need(sgd_ofs, sgd_len, "the BasisLZ global data") || sgd_len < 20 || (sgd_len - 20) / 20 < n_images) {
        if (error.empty()) error = fmt("truncated or corrupt file: the BasisLZ global data of %llu bytes cannot hold %llu image descriptors", (unsigned long long)sgd_len, (unsigned long long)n_images);
        return false;
    }
    f.container = 1; f.tex_type = faces == 6 ? 2 : (layers ? 1 : 0); f.srgb = v.data[dfd_ofs + 14] == 2;
    f.width = width; f.height = height; f.levels = levels; f.layers = (uint32_t)n_layers; f.faces = faces;
    f.num_endpoints = (uint32_t)v.le(sgd_ofs, 2); f.num_selectors = (uint32_t)v.le(sgd_ofs + 2, 2);
    const uint64_t ep_len = v.le(sgd_ofs + 4, 4), sel_len = v.le(sgd_ofs + 8, 4), tab_len = v.le(sgd_ofs + 12, 4), ext_len = v.le(sgd_ofs + 16, 4);
    const uint64_t ep_ofs = sgd_ofs + 20 + 20 * n_images;
    if (ep_len + sel_len + tab_len + ext_len > sgd_len - 20 - 20 * n_images) { error = "truncated or corrupt file: the BasisLZ global data is smaller than the palettes and tables it announces"; return false; }
    sec.endpoints = span{v.data + ep_ofs, ep_len}; sec.selectors = span{v.data + ep_ofs + ep_len, sel_len}; sec.tables = span{v.data + ep_ofs + ep_len + sel_len, tab_len};
    for (uint32_t l = 0; l < levels; l++) {
        const uint64_t lofs = v.le(80 + 24ull * l, 8), llen = v.le(88 + 24ull * l, 8);
        if (!v.need(lofs, llen, fmt("level %u", l).c_str())) return false;
        const uint32_t w = std::max(width >> l, 1u), h = std::max(height >> l, 1u);
        for (uint64_t k = 0; k < per_level; k++) {
            const uint64_t at = sgd_ofs + 20 + 20 * (l * per_level + k);
            const uint32_t iflags = (uint32_t)v.le(at, 4);
            const uint64_t rgb_ofs = v.le(at + 4, 4), rgb_len = v.le(at + 8, 4), a_ofs = v.le(at + 12, 4), a_len = v.le(at + 16, 4);
            if (iflags & 2u) { error = "video files are not supported: a P-frame's blocks may repeat the previous frame's indices, which this reader does not keep"; return false; }
            if (!rgb_len || rgb_ofs > llen || rgb_len > llen - rgb_ofs || a_ofs > llen || a_len > llen - a_ofs) {
                error = fmt("truncated or corrupt file: level %u, image %llu: its slices lie outside the level's %llu bytes", l, (unsigned long long)k, (unsigned long long)llen);
                return false;
            }
            etc1s_image im;
            im.level = l; im.layer = (uint32_t)(k / faces); im.face = (uint32_t)(k % faces);
            im.width = w; im.height = h; im.num_blocks_x = (w + 3) / 4; im.num_blocks_y = (h + 3) / 4;
            im.rgb_ofs = lofs + rgb_ofs; im.rgb_len = rgb_len; im.alpha_ofs = lofs + a_ofs; im.alpha_len = a_len;
            f.images.push_back(im);
        }
    }
    return finish_image_list(f, error);
}

}  // namespace

bool decode_etc1s_file(const uint8_t* data, uint64_t size, bool header_only, etc1s_file& f, std::string& error) {
    f = etc1s_file();
    error.clear();
    static const uint8_t ktx2_magic[12] = {0xAB, 0x4B, 0x54, 0x58, 0x20, 0x32, 0x30, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A};
    if (!data && size) { error = "null data"; return false; }
    const file_view v{data, size, &error};
    sections sec;
    if (size >= 12 && !std::memcmp(data, ktx2_magic, 12)) { if (!parse_ktx2(v, f, sec)) return false; }
    else if (size >= 2 && data[0] == 's' && data[1] == 'B') { if (!parse_basis(v, f, sec)) return false; }
    else { error = size < 12 ? fmt("truncated file: %llu bytes hold no container signature", (unsigned long long)size) : std::string("neither a .basis nor a .ktx2 file"); return false; }
    if (!f.num_endpoints || !f.num_selectors || f.num_endpoints > kMaxPaletteEntries || f.num_selectors > kMaxPaletteEntries) {
        error = fmt("palettes of %u endpoints and %u selectors", f.num_endpoints, f.num_selectors);
        return false;
    }
    // what sizes the index arrays is bounded before anything is allocated
    for (const etc1s_image& im : f.images)
        if (im.width > kMaxDimension || im.height > kMaxDimension) { error = fmt("level %u, layer %u, face %u: %u x %u texels is more than this reader takes", im.level, im.layer, im.face, im.width, im.height); return false; }
    if (f.total_blocks > kMaxTotalBlocks) { error = fmt("%llu blocks in one file is more than this reader takes", (unsigned long long)f.total_blocks); return false; }
    if (header_only) return true;

    if (!decode_endpoint_palette(sec.endpoints, f.num_endpoints, f.endpoint_palette, error) || !decode_selector_palette(sec.selectors, f.num_selectors, f.selector_palette, error)) return false;
    slice_models models;
    if (!decode_tables(sec.tables, models, error)) return false;

    std::vector<slice_job> jobs;
    for (size_t i = 0; i < f.images.size(); i++) {
        const etc1s_image& im = f.images[i];
        slice_job j;
        j.nbx = im.num_blocks_x; j.nby = im.num_blocks_y; j.image = (uint32_t)i;
        j.bits = span{data + im.rgb_ofs, im.rgb_len}; j.first_block = im.first_block; j.alpha = false;
        jobs.push_back(j);
        if (im.alpha_len) { j.bits = span{data + im.alpha_ofs, im.alpha_len}; j.first_block = im.alpha_first_block; j.alpha = true; jobs.push_back(j); }
    }
    f.endpoint_indices.assign(f.total_blocks, 0);
    f.selector_indices.assign(f.total_blocks, 0);
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&]() {   // nothing thrown leaves a worker: a failed allocation inside a slice becomes that slice's error
        for (size_t k; !failed.load(std::memory_order_relaxed) && (k = next.fetch_add(1)) < jobs.size();) {
            bool ok = false;
            try {
                ok = decode_slice(jobs[k], models, f.num_endpoints, f.num_selectors, f.endpoint_indices.data() + jobs[k].first_block, f.selector_indices.data() + jobs[k].first_block);
            } catch (const std::exception& e) {
                try { jobs[k].error = std::string("out of memory or internal error while decoding a slice: ") + e.what(); } catch (...) { }
            }
            if (!ok) failed.store(true);
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t threads = std::min<size_t>({jobs.size(), (size_t)kMaxDecodeThreads, (size_t)hw});
    std::vector<std::thread> pool;
    try {
        for (size_t t = 1; t < threads; t++) pool.emplace_back(work);
    } catch (const std::exception&) { }   // no more threads to be had: the ones that started and this one share the slices
    work();
    for (std::thread& t : pool) t.join();
    if (failed.load()) {
        bool said = false;
        for (const slice_job& j : jobs) said = said || !j.error.empty();
        if (!said) { error = "out of memory while decoding a slice"; return false; }
    }
    for (const slice_job& j : jobs) if (!j.error.empty()) { error = j.error; return false; }   // the first failing slice in file order, whichever thread met it
    return true;
}

}  // namespace bu

// ---------------------------------------------------------------- C ABI (include/basisu_hip_etc1s_decode.h)
struct bu_etc1s_file { bu::etc1s_file f; };

extern "C" {

bu_etc1s_file* bu_etc1s_decode_file(const void* data, uint64_t size, uint32_t flags, char* err, uint32_t err_cap) {
    if (err && err_cap) err[0] = 0;
    std::string error;
    bu_etc1s_file* h = nullptr;
    try {
        h = new bu_etc1s_file();
        if (bu::decode_etc1s_file(static_cast<const uint8_t*>(data), size, (flags & BU_ETC1S_DECODE_HEADER_ONLY) != 0, h->f, error)) return h;
    } catch (const std::exception& e) {
        error = std::string("out of memory or internal error: ") + e.what();
    }
    delete h;
    if (err && err_cap) std::snprintf(err, err_cap, "%s", error.c_str());
    return nullptr;
}

void bu_etc1s_file_destroy(bu_etc1s_file* h) { delete h; }

void bu_etc1s_file_get_info(const bu_etc1s_file* h, bu_etc1s_file_info* out) {
    if (!h || !out) return;
    const bu::etc1s_file& f = h->f;
    *out = bu_etc1s_file_info{f.container, f.tex_type, f.width, f.height, f.levels, f.layers, f.faces, f.has_alpha_slices ? 1u : 0u, f.srgb ? 1u : 0u,
                              f.num_endpoints, f.num_selectors, (uint32_t)f.images.size(), f.total_blocks};
}

uint32_t bu_etc1s_file_get_images(const bu_etc1s_file* h, bu_etc1s_image* out, uint32_t cap) {
    if (!h) return 0;
    const uint32_t n = (uint32_t)h->f.images.size();
    for (uint32_t i = 0; out && i < n && i < cap; i++) {
        const bu::etc1s_image& im = h->f.images[i];
        out[i] = bu_etc1s_image{im.level, im.layer, im.face, im.width, im.height, im.num_blocks_x, im.num_blocks_y, 0, im.first_block, im.alpha_first_block};
    }
    return n;
}

const uint8_t* bu_etc1s_file_endpoint_palette(const bu_etc1s_file* h) { return h ? h->f.endpoint_palette.data() : nullptr; }
const uint32_t* bu_etc1s_file_selector_palette(const bu_etc1s_file* h) { return h ? h->f.selector_palette.data() : nullptr; }
const uint16_t* bu_etc1s_file_endpoint_indices(const bu_etc1s_file* h) { return h ? h->f.endpoint_indices.data() : nullptr; }
const uint16_t* bu_etc1s_file_selector_indices(const bu_etc1s_file* h) { return h ? h->f.selector_indices.data() : nullptr; }

}  // extern "C"
