"""The block decode core (csrc/block_unpack.h) built with g++ against the reference's known answers (tests/golden/block_unpack_vectors.npz, written by
tools/gen_golden_block_unpack.py from basisu::unpack_block): no GPU anywhere in this file."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import block_unpack_helpers as B
import image_metrics_helpers as M
import transcode_helpers as T
from basis_universal_amd import transcode

ROOT = pathlib.Path(__file__).resolve().parent.parent
FORMATS = [B.BC1, B.BC3, B.BC4, B.BC5, B.BC7]


def _members():
    return sorted(B.golden()[1]["members"].items())


@pytest.mark.parametrize("name", [n for n, _ in _members()])
def test_host_core_equals_the_reference_on_every_golden_block(name):
    """Every block compared, none left out: validity flags equal, every block the reference accepts texel-equal, every block it refuses zero-filled (where the
    reference keeps whatever its caller's buffer held: its pre-fill, in the fixture)."""
    arrays, meta = B.golden()
    fmt = meta["members"][name]["format"]
    blocks, want, want_ok = arrays[name + "_blocks"], arrays[name + "_texels"], arrays[name + "_ok"]
    assert blocks.shape == (meta["members"][name]["blocks"], B.BYTES[fmt]) and want.shape == (blocks.shape[0], 16, 4)
    got, got_ok = B.host_unpack(blocks, fmt)
    assert (got_ok == want_ok).all(), (name, np.flatnonzero(got_ok != want_ok)[:8])
    refused = want_ok == 0
    assert int(refused.sum()) == meta["members"][name]["refused"]
    assert (got[refused] == 0).all(), name
    assert (want[refused] == np.array([0, 0, 0, 255], np.uint8)).all(), "the reference left its pre-fill in a block it refused"
    bad = np.flatnonzero((got[~refused] != want[~refused]).any(axis=(1, 2)))
    if bad.size:
        i = np.flatnonzero(~refused)[bad[0]]
        raise AssertionError(f"{name}: {bad.size} of {blocks.shape[0]} blocks differ; first: block {i} {blocks[i].tobytes().hex()} got {got[i].tobytes().hex()} "
                             f"reference {want[i].tobytes().hex()}")


def test_the_fixture_covers_what_it_says_it_covers():
    """Counted from the blocks themselves: every BC7 mode, every partition of the modes that have one, every (rotation, index selection) setting, all-zero and all-one
    endpoint fields per mode, the 16 reserved-mode blocks; the three endpoint orders of BC1 (each with index 3 in use) and BC4, BC4's (0, 255) and (255, 0),
    BC3 colour halves that plain BC1 would decode with three colours."""
    arrays, meta = B.golden()
    seen = B.check_coverage(arrays, meta)
    assert [seen[f"bc7 mode {m}"] for m in range(8)] == [meta["bc7_counts"][str(m)] for m in range(8)]
    assert sorted(set(B.bc7_modes(arrays["bc7_blocks"]).tolist())) == [-1, 0, 1, 2, 3, 4, 5, 6, 7]
    # and the encoder-made BC7 blocks are of the modes the UASTC transcoder writes
    assert set(B.bc7_modes(arrays["level2_bc7_blocks"]).tolist()) <= {1, 2, 3, 5, 6, 7}


def test_bc3_and_bc5_are_their_halves():
    for fmt in (B.BC3, B.BC5):
        blocks, _, _ = B.format_set(fmt)
        got, ok = B.host_unpack(blocks, fmt)
        assert ok.all()
        first, _ = B.host_unpack(blocks[:, :8], B.BC4)
        if fmt == B.BC3:
            assert (got[..., 3] == first[..., 0]).all(), "BC3 alpha is BC4 of bytes 0-7"
            assert (got[..., :3] == B.host_bc1_four_colour(blocks[:, 8:])[..., :3]).all(), "BC3 colour is the four-colour decode of bytes 8-15"
            plain, _ = B.host_unpack(blocks[:, 8:], B.BC1)
            three = B.endpoint_orders(blocks, 64, 16) <= 0
            assert three.sum() >= 64 and (plain[three][..., :3] != got[three][..., :3]).any(), "and that differs from plain BC1 where low <= high"
            assert (plain[~three][..., :3] == got[~three][..., :3]).all()
        else:
            second, _ = B.host_unpack(blocks[:, 8:], B.BC4)
            assert (got[..., 0] == first[..., 0]).all() and (got[..., 1] == second[..., 0]).all(), "BC5 is two BC4s"
            assert (got[..., 2] == 0).all() and (got[..., 3] == 255).all()
    blocks, _, _ = B.format_set(B.BC4)
    got, _ = B.host_unpack(blocks, B.BC4)
    assert (got[..., 1:3] == 0).all() and (got[..., 3] == 255).all(), "BC4 writes R only"


def _uastc_images(raw):
    info = transcode.read_uastc_file(raw)
    for im in info["images"]:
        yield im, np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16)


def _host_bc7_raster(im, blocks):
    bc7, ok = T.host_transcode(blocks, T.BC7)
    assert ok.all()
    texels, ok = B.host_unpack(bc7, B.BC7)
    assert ok.all()
    return np.ascontiguousarray(B.to_raster(texels, im["num_blocks_x"], im["num_blocks_y"], im["width"], im["height"]))


def _host_lines(src, dec):
    hist, _, _ = M.host_counts(np.ascontiguousarray(src), dec)
    h, w = dec.shape[:2]
    return {line: M.host_reduce(hist, total, first, w, h, use_601) for line, (first, total, use_601) in M.LINES.items()}


@pytest.mark.parametrize("case", ["uastc_alpha_ktx2", "uastc_o20_basis", "uastc_mip_basis"])
def test_bc7_stats_on_the_host_match_what_the_reference_tool_printed(case):
    """The golden UASTC file -> host BC7 transcode -> host unpack -> crop -> the host image metrics, against the `BC7 ...` lines the tool printed. Of the mip case
    only level 0 has a source without the device's mip generator; tests/test_gpu_block_unpack.py checks every level."""
    arrays, meta = B.golden_stats()
    entry = next(c for c in meta["cases"] if c["name"] == case)
    shared, _ = M.golden()
    raw = (shared if entry["in_image_stats_vectors"] else arrays)["file_" + case].tobytes()
    src = (shared if entry["in_image_stats_vectors"] else arrays)["src_" + case]
    images = list(_uastc_images(raw))
    assert len(images) == entry["slices"] == arrays["stats_" + case].shape[0]
    im, blocks = images[0]
    assert im["level"] == 0
    M.assert_close_to_printed(_host_lines(src, _host_bc7_raster(im, blocks)), arrays["stats_" + case][0], case)


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "block_unpack.h"
using namespace bu_unpack;
static unsigned long long run(const unsigned char* b, unsigned fmt, unsigned* refused) {
    // exact-size copies on the heap: a read one byte past the block, or a write past the 64 texel bytes, is a sanitizer report
    const unsigned unit = unpack_bytes_per_block(fmt);
    unsigned char* in = (unsigned char*)std::malloc(unit);
    unsigned char* out = (unsigned char*)std::malloc(64);
    std::memcpy(in, b, unit);
    bool ok = false;
    switch (fmt) {
    case UF_BC1: ok = unpack_block_bc1(in, out); break;
    case UF_BC3: ok = unpack_block_bc3(in, out); break;
    case UF_BC4: ok = unpack_block_bc4(in, out); break;
    case UF_BC5: ok = unpack_block_bc5(in, out); break;
    default: ok = unpack_block_bc7(in, out); break;
    }
    unsigned long long sum = 0;
    for (int i = 0; i < 64; i++) sum = sum * 31 + out[i];
    if (!ok) (*refused)++;
    std::free(in); std::free(out);
    return sum;
}
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> data;
    unsigned char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    const unsigned formats[5] = { UF_BC1, UF_BC3, UF_BC4, UF_BC5, UF_BC7 };
    unsigned long long sum = 0;
    unsigned refused = 0, golden = 0;
    // every golden block (the file is their bytes end to end, 16 per block, 8-byte blocks padded) through all five decoders
    for (size_t at = 0; at + 16 <= data.size(); at += 16, golden++)
        for (unsigned k = 0; k < 5; k++) sum += run(&data[at], formats[k], &refused);
    const unsigned total = (unsigned)std::atoi(argv[2]);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (unsigned i = 0; i < total; i++) {
        unsigned char b[16];
        const unsigned long long lo = next(), hi = next();
        std::memcpy(b, &lo, 8); std::memcpy(b + 8, &hi, 8);
        for (unsigned k = 0; k < 5; k++) sum += run(b, formats[k], &refused);
    }
    std::printf("golden %u random %u refused %u sum %llu\n", golden, total, refused, sum);
    return 0;
}
"""


def test_every_decoder_under_host_sanitizers(tmp_path):
    """block_unpack.h built with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program (host code, CPU only): every golden block and 100,000
    random 16-byte blocks from a fixed seed through all five decoders, and no sanitizer speaks."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer harness"
    (tmp_path / "main.cpp").write_text(SANITIZER_MAIN)
    exe = tmp_path / "unpack_all"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", str(ROOT / "basis_universal_amd" / "csrc"), "-o", str(exe), str(tmp_path / "main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    arrays, meta = B.golden()
    padded = []
    for name in sorted(meta["members"]):
        b = arrays[name + "_blocks"]
        padded.append(np.concatenate([b, np.zeros((b.shape[0], 16 - b.shape[1]), np.uint8)], 1))
    allb = np.concatenate(padded)
    (tmp_path / "blocks.bin").write_bytes(allb.tobytes())
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    r = subprocess.run([str(exe), str(tmp_path / "blocks.bin"), "100000"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    words = r.stdout.split()
    assert (int(words[1]), int(words[3])) == (allb.shape[0], 100000), r.stdout
    assert int(words[5]) > 0   # some block was refused: byte 0 == 0 occurs among the golden blocks and about once in 256 random ones
