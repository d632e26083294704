// ssim_host_check.cpp -- a stand-alone host program over csrc/ssim.h and csrc/ssim_reduce.h for a sanitizer run (no GPU, nothing loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o ssim_host_check tools/ssim_host_check.cpp && ./ssim_host_check
// For every size it (1) computes the smap values straight from the rasters with clamped coordinates, (2) computes them again the way the map kernel's workgroup does --
// a 16x16 tile and its 5-pixel halo staged into a heap array of exactly the kernel's LDS size (26 rows, 48 words apart), every lane reading through the same pointer
// arithmetic -- and (3) sums every plane serially and with the chunked walk. (1) and (2), and the two sums, must agree bit for bit; the sanitizers watch the indexing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../basis_universal_amd/csrc/ssim_reduce.h"

static const int kTile = 16, kSpan = kTile + 2 * bu::SSIM_RADIUS, kRow = 48;
static const uint32_t kChunk = 256;

template <int C>
static void direct(const std::vector<uint32_t>& a, uint32_t pitch_a, const std::vector<uint32_t>& b, uint32_t pitch_b, int w, int h, const bu::ssim_weights& k, std::vector<float>& planes) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float out[C];
            bu::ssim_pixel<C>([&](int xd, int yd, uint32_t& sa, uint32_t& sb) {
                const int cx = x + xd < 0 ? 0 : (x + xd >= w ? w - 1 : x + xd), cy = y + yd < 0 ? 0 : (y + yd >= h ? h - 1 : y + yd);
                sa = bu::ssim_sample<C>(a[(size_t)cy * pitch_a + cx]);
                sb = bu::ssim_sample<C>(b[(size_t)cy * pitch_b + cx]);
            }, k, out);
            for (int c = 0; c < C; c++) planes[(size_t)c * w * h + (size_t)y * w + x] = out[c];
        }
}

template <int C>
static void tiled(const std::vector<uint32_t>& a, uint32_t pitch_a, const std::vector<uint32_t>& b, uint32_t pitch_b, int w, int h, const bu::ssim_weights& k, std::vector<float>& planes) {
    for (int y0 = 0; y0 < h; y0 += kTile)
        for (int x0 = 0; x0 < w; x0 += kTile) {
            std::unique_ptr<uint32_t[]> ta(new uint32_t[kSpan * kRow]), tb(new uint32_t[kSpan * kRow]);   // heap, exact size: an index past the end is reported
            for (int i = 0; i < kSpan * kSpan; i++) {
                const int ty = i / kSpan, tx = i - ty * kSpan;
                int gx = x0 + tx - bu::SSIM_RADIUS, gy = y0 + ty - bu::SSIM_RADIUS;
                gx = gx < 0 ? 0 : (gx > w - 1 ? w - 1 : gx); gy = gy < 0 ? 0 : (gy > h - 1 ? h - 1 : gy);
                ta[ty * kRow + tx] = bu::ssim_sample<C>(a[(size_t)gy * pitch_a + gx]);
                tb[ty * kRow + tx] = bu::ssim_sample<C>(b[(size_t)gy * pitch_b + gx]);
            }
            for (int t = 0; t < kTile * kTile; t++) {
                const int lx = t % kTile, ly = t / kTile, x = x0 + lx, y = y0 + ly;
                if (x >= w || y >= h) continue;
                const uint32_t* pa = ta.get() + (ly + bu::SSIM_RADIUS) * kRow + lx + bu::SSIM_RADIUS;
                const uint32_t* pb = tb.get() + (ly + bu::SSIM_RADIUS) * kRow + lx + bu::SSIM_RADIUS;
                float out[C];
                bu::ssim_pixel<C>([&](int xd, int yd, uint32_t& sa, uint32_t& sb) { sa = pa[yd * kRow + xd]; sb = pb[yd * kRow + xd]; }, k, out);
                for (int c = 0; c < C; c++) planes[(size_t)c * w * h + (size_t)y * w + x] = out[c];
            }
        }
}

static float chunked(const float* v, uint32_t n) {
    const uint32_t chunks = (n + kChunk - 1) / kChunk;
    std::vector<bu::ssim_chunk> sm(chunks);
    double prefix = 0.0;
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t i0 = c * kChunk, len = n - i0 < kChunk ? n - i0 : kChunk;
        sm[c] = bu::ssim_chunk_build(v + i0, len, prefix);
        for (uint32_t i = 0; i < len; i++) prefix += (double)v[i0 + i];
    }
    uint32_t state = 0, walked = 0;
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t i0 = c * kChunk;
        state = bu::ssim_chunk_walk(state, sm[c], v + i0, n - i0 < kChunk ? n - i0 : kChunk, &walked);
    }
    return bu::ssim_float(state) / static_cast<float>(n);
}

static int check(int w, int h, uint32_t pad_a, uint32_t pad_b) {
    const uint32_t pitch_a = w + pad_a, pitch_b = w + pad_b;
    std::vector<uint32_t> a((size_t)(h - 1) * pitch_a + w), b((size_t)(h - 1) * pitch_b + w);   // a raster ends with its last pixel: a read into the last row's padding is reported
    uint32_t s = 12345u + w * 131u + h;
    for (auto& p : a) { s = s * 1664525u + 1013904223u; p = s; }
    for (size_t i = 0; i < b.size(); i++) { s = s * 1664525u + 1013904223u; b[i] = (i % 7) ? a[i % a.size()] ^ (s & 0x07030503u) : s; }
    bu::ssim_weights k;
    bu::ssim_gaussian_weights(k.w);
    const size_t n = (size_t)w * h;
    std::vector<float> d(6 * n), t(6 * n);
    direct<4>(a, pitch_a, b, pitch_b, w, h, k, d);
    tiled<4>(a, pitch_a, b, pitch_b, w, h, k, t);
    std::vector<float> d2(2 * n), t2(2 * n);
    direct<2>(a, pitch_a, b, pitch_b, w, h, k, d2);
    tiled<2>(a, pitch_a, b, pitch_b, w, h, k, t2);
    memcpy(d.data() + 4 * n, d2.data(), 2 * n * sizeof(float));
    memcpy(t.data() + 4 * n, t2.data(), 2 * n * sizeof(float));
    int bad = memcmp(d.data(), t.data(), d.size() * sizeof(float)) != 0;
    for (int p = 0; p < 6; p++) {
        const float serial = bu::ssim_avg(d.data() + p * n, n), walk = chunked(t.data() + p * n, (uint32_t)n);
        bad |= bu::ssim_bits(serial) != bu::ssim_bits(walk);
        printf("%dx%d plane %d mean %f\n", w, h, p, serial);
    }
    return bad;
}

int main() {
    int bad = check(1, 1, 0, 0) | check(5, 7, 3, 0) | check(20, 28, 0, 5) | check(33, 17, 1, 2) | check(300, 3, 0, 0);
    printf(bad ? "MISMATCH\n" : "ssim_host_check: tiled = direct and chunked = serial at every size\n");
    return bad;
}
