// etc1s_decode.h -- the reader that matches etc1s_backend.cpp's writers: an ETC1S .basis / BasisLZ .ktx2 file in, the two palettes and every slice's per-block
// endpoint and selector indices out (include/basisu_hip_etc1s_decode.h is its C view). The walk inside a slice is serial like the backend's -- every block's
// symbols depend on the blocks before it -- so this is host code; slices are independent and go to separate threads.
//
//   bit_reader / huffman_decoder  the inverse of entropy.h's bit_writer / huffman_table       (= bitwise_decoder, huffman_decoding_table; transcoder_internal.h:293-751)
//   decode_endpoint_palette       the inverse of etc1s_backend::encode_endpoint_palette        (= decode_palettes, transcoder.cpp:8257-8343)
//   decode_selector_palette       the inverse of etc1s_backend::encode_selector_palette        (= decode_palettes, transcoder.cpp:8345-8438)
//   decode_slice                  the inverse of etc1s_backend::encode_image's per-slice coding (= the symbol half of transcode_slice, transcoder.cpp:8659-8841)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bu {

struct etc1s_image {
    uint32_t level = 0, layer = 0, face = 0, width = 0, height = 0, num_blocks_x = 0, num_blocks_y = 0;
    uint64_t first_block = ~0ull, alpha_first_block = ~0ull;
    // where the slices' bytes are in the file
    uint64_t rgb_ofs = 0, rgb_len = 0, alpha_ofs = 0, alpha_len = 0;
};

struct etc1s_file {
    uint32_t container = 0, tex_type = 0, width = 0, height = 0, levels = 0, layers = 0, faces = 1;
    bool has_alpha_slices = false, srgb = false;
    uint32_t num_endpoints = 0, num_selectors = 0;
    uint64_t total_blocks = 0;
    std::vector<etc1s_image> images;
    std::vector<uint8_t> endpoint_palette;    // 4 per entry: r5, g5, b5, intensity table
    std::vector<uint32_t> selector_palette;   // selector of texel (x, y) at bits 2 * (y * 4 + x)
    std::vector<uint16_t> endpoint_indices, selector_indices;
};

// false: `error` says why. header_only: stop after the containers' descriptors.
bool decode_etc1s_file(const uint8_t* data, uint64_t size, bool header_only, etc1s_file& out, std::string& error);

}  // namespace bu
