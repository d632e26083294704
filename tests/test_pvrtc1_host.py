"""Host half of the PVRTC1 4bpp targets: the CPU restatement of tests/pvrtc1_helpers.py against the reference tool's bytes (tests/golden/pvrtc1_vectors.npz), the
coverage the fixture was written under, the code and address rules of basis_universal_amd/csrc/pvrtc1.h (compiled for the host under AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone program, tools/pvrtc1_sanitize.cpp) against brute force, and the Python layer's layout and refusals. No GPU."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import multi_image_helpers as M
import pvrtc1_helpers as P
from basis_universal_amd import transcode as T

ROOT = pathlib.Path(__file__).resolve().parent.parent
ROUTES = ("etc1s_rgb", "etc1s_rgba", "uastc_rgb", "uastc_rgba")
RESERVED_MODE_BYTE = P.reserved_mode_byte()   # a first byte no UASTC mode code matches: the block is refused


def _files():
    _, meta = P.golden()
    return [f["name"] for f in meta["files"]]


def _images(name):
    """every image of a golden file -> [(key, blocks-or-decoded, image, has alpha)]; ETC1S: the decoded file, UASTC: the image's (n, 16) blocks"""
    arrays, meta = P.golden()
    entry = next(f for f in meta["files"] if f["name"] == name)
    raw = arrays["file_" + name].tobytes()
    if entry["codec"] == "etc1s":
        dec = T.decode_etc1s_file(raw)
        images = [(dec, im, im["has_alpha"]) for im in dec["images"]]
    else:
        info = T.read_uastc_file(raw)
        images = [(np.frombuffer(raw, np.uint8, im["length"], im["offset"]).reshape(-1, 16), im, info["has_alpha"]) for im in info["images"]]
    assert [[im["level"], im["layer"], im["face"], im["width"], im["height"]] for _, im, _ in images] == entry["images"]
    return entry["codec"], [(P.image_key(name, im["level"], im["layer"], im["face"]), src, im, alpha) for src, im, alpha in images]


def _restated(codec, src, im, target):
    if codec == "etc1s":
        return P.etc1s_image_blocks(src, im, target)
    return P.uastc_blocks(src, im["num_blocks_x"], im["num_blocks_y"], target)[0]


@pytest.mark.parametrize("name", _files())
def test_restatement_reproduces_every_golden_block(name):
    """PVRTC1_4_RGB and PVRTC1_4_RGBA, every image of every golden file, byte for byte; RGBA asked of a source without alpha is the RGB route"""
    arrays, _ = P.golden()
    codec, images = _images(name)
    for key, src, im, alpha in images:
        for short, target in P.TARGETS.items():
            got, want = _restated(codec, src, im, target if alpha else P.RGB), arrays[key + "_" + short]
            bad = np.flatnonzero((got != want).any(1))
            assert got.shape == want.shape and bad.size == 0, (key, short, bad[:8])
        if not alpha:
            assert (arrays[key + "_rgb"] == arrays[key + "_rgba"]).all(), key


def test_golden_meets_the_coverage_conditions():
    """Counted by the restatement while the generator wrote the file. One condition is dropped by name: a block whose LOW endpoint is opaque and whose HIGH endpoint
    is translucent cannot exist. The low endpoint is opaque only where the block's lowest alpha is 255 (floor: the one value code 8 expands to); the highest alpha is
    then 255 too (a minimum is not above a maximum; ETC1S bounds are the block colours of the lowest and highest selector in use, which ascend), and 255 ceils to
    code 8. The fixture counts 0 of them. ca > cb never occurs either (floor <= ceil per block, and the weights are not negative); the kernels keep the branch."""
    _, meta = P.golden()
    stats = meta["stats"]
    assert sorted(stats) == sorted(ROUTES)
    for route in ROUTES:
        s = stats[route]
        assert min(s["modulation"]) > 0, (route, s["modulation"])
        assert min(s["wrapped"].values()) > 0, (route, s["wrapped"])
        assert s["dl_zero_p_positive"] > 0 and s["dl_zero_p_not_positive"] > 0, (route, s)
        assert s["ca_above_cb"] == 0, (route, s)
        f = s["endpoint_formats"]
        if route.endswith("rgba"):
            assert f["opaque_opaque"] > 0 and f["translucent_opaque"] > 0 and f["translucent_translucent"] > 0 and f["opaque_translucent"] == 0, (route, f)
        else:
            assert f["opaque_opaque"] == s["blocks"], (route, f)
    for route in ("etc1s_rgb", "etc1s_rgba"):
        assert all(stats[route][f"p_equals_{k}dl"] > 0 for k in (3, 8, 13)), (route, stats[route])
    own = meta["etc1s_coverage"]["stats"]   # the synthetic state alone holds them too: it is where they were searched for
    assert all(own[route][f"p_equals_{k}dl"] > 0 for route in own for k in (3, 8, 13)), own


def test_restatement_codes_against_the_definitions():
    """the restatement's own tables: expansions by explicit bit replication, floor / ceil against their defining inequalities for all 256 inputs"""
    assert [int(v) for v in P.EXPAND[5]] == [(c << 3) | (c >> 2) for c in range(32)]
    assert [int(v) for v in P.EXPAND[4]] == [(((c << 1) | (c >> 3)) << 3) | (((c << 1) | (c >> 3)) >> 2) for c in range(16)]
    assert [int(v) for v in P.EXPAND[3]] == [(((c << 2) | (c >> 1)) << 3) | (((c << 2) | (c >> 1)) >> 2) for c in range(8)]
    assert [int(v) for v in P.EXPAND["alpha"]] == [((2 * a) << 4) | (2 * a) for a in range(8)] + [255]
    for kind, e in P.EXPAND.items():
        assert e[0] == 0 and e[-1] == 255 and (np.diff(e) > 0).all()
        for v in range(256):
            f, c = int(P.FLOOR[kind][v]), int(P.CEIL[kind][v])
            assert e[f] <= v and (f == e.size - 1 or e[f + 1] > v), (kind, v, f)
            assert e[c] >= v and (c == 0 or e[c - 1] < v), (kind, v, c)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tools/pvrtc1_sanitize.cpp built once per run by g++ with both sanitizers, statically linked runtimes: a plain executable, nothing of it is loaded here"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the sanitizer program"
    out = tmp_path_factory.mktemp("pvrtc1_sanitize") / "pvrtc1_sanitize"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover", "-fno-omit-frame-pointer",
                        "-ffp-contract=off", "-o", str(out), str(ROOT / "tools" / "pvrtc1_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(program, tmp_path, mode, words=None):
    """one run of the program: `words` (u32) in, the output file's u32 words back; no sanitizer may speak"""
    args = [str(program), mode]
    if words is not None:
        np.ascontiguousarray(words, np.uint32).tofile(tmp_path / "in.bin")
        args.append(str(tmp_path / "in.bin"))
    args.append(str(tmp_path / "out.bin"))
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    r = subprocess.run(args, capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (mode, r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return np.fromfile(tmp_path / "out.bin", np.uint32)


def test_kernel_code_rules_against_brute_force(program, tmp_path):
    """floor / ceil / expansion as the kernels compute them (closed forms), for all 256 inputs and every code: floor = the largest code whose expansion is <= v,
    ceil = the smallest whose expansion is >= v, the expansions by bit replication"""
    out = _run(program, tmp_path, "codes")
    rows, rest = out[:256 * 8].reshape(256, 8).astype(np.int64), out[256 * 8:].astype(np.int64)
    for col, (table, kind) in enumerate(((P.FLOOR, 5), (P.CEIL, 5), (P.FLOOR, 4), (P.CEIL, 4), (P.FLOOR, 3), (P.CEIL, 3), (P.FLOOR, "alpha"), (P.CEIL, "alpha"))):
        assert (rows[:, col] == table[kind]).all(), (col, kind, np.flatnonzero(rows[:, col] != table[kind])[:8])
    assert (rest == np.concatenate([P.EXPAND[5], P.EXPAND[4], P.EXPAND[3], P.EXPAND["alpha"]])).all()


def test_morton_address_against_a_bit_by_bit_interleave(program, tmp_path):
    """every (nbx, nby) in {1, 2, 4, ..., 1024}^2: the four corners and 64 random blocks each; and a permutation of the image's blocks for every size up to 64x64"""
    rng = np.random.default_rng(8)
    sizes = [1 << k for k in range(11)]
    recs = []
    for nbx in sizes:
        for nby in sizes:
            pts = [(0, 0), (nbx - 1, 0), (0, nby - 1), (nbx - 1, nby - 1)] + [(int(rng.integers(0, nbx)), int(rng.integers(0, nby))) for _ in range(64)]
            recs += [(x, y, nbx, nby) for x, y in pts]
    whole = [(nbx, nby) for nbx in sizes[:7] for nby in sizes[:7]]
    for nbx, nby in whole:
        recs += [(x, y, nbx, nby) for y in range(nby) for x in range(nbx)]
    recs = np.array(recs, np.uint32)
    got = _run(program, tmp_path, "morton", recs)
    want = np.array([P.interleave_bit_by_bit(int(x), int(y), int(nbx), int(nby)) for x, y, nbx, nby in recs], np.uint32)
    assert (got == want).all(), recs[np.flatnonzero(got != want)[:8]]
    at = 121 * 68
    for nbx, nby in whole:
        n = nbx * nby
        assert sorted(got[at:at + n].tolist()) == list(range(n)), (nbx, nby)
        assert (got[at:at + n].reshape(nby, nbx) == P.morton_addresses(nbx, nby)).all(), (nbx, nby)   # the restatement's vectorised form is the same map
        at += n
    assert at == got.size


def _etc1s_words(ep_pal, sel_pal, idx, nbx, nby, alpha):
    pal = np.ascontiguousarray(ep_pal, np.uint8).reshape(-1, 4).view(np.uint32).reshape(-1)
    idx = np.stack([np.asarray(a, np.uint32).reshape(-1) for a in idx[:4 if alpha else 2]], 1).reshape(-1)
    return np.concatenate([np.array([nbx, nby, int(alpha), pal.size, np.asarray(sel_pal).size], np.uint32), pal, np.asarray(sel_pal, np.uint32).reshape(-1), idx])


def _uastc_words(blocks, nbx, nby, alpha):
    return np.concatenate([np.array([nbx, nby, int(alpha)], np.uint32), np.ascontiguousarray(blocks, np.uint8).reshape(-1).view(np.uint32)])


def test_kernel_block_code_under_host_sanitizers_equals_the_goldens_and_the_restatement(program, tmp_path):
    """Both passes as the kernels run them (pvrtc1.h; for UASTC behind the unpacker of uastc_transcode.h), over every image of every golden file in both targets
    and over random states of every small shape, some with planted invalid blocks: no sanitizer speaks, every byte is the reference tool's / the restatement's."""
    arrays, _ = P.golden()
    for name in _files():
        codec, images = _images(name)
        for key, src, im, has_alpha in images:
            nbx, nby = im["num_blocks_x"], im["num_blocks_y"]
            for short, target in P.TARGETS.items():
                alpha = has_alpha and target == P.RGBA
                if codec == "etc1s":
                    words = _etc1s_words(src["endpoint_palette"], src["selector_palette"], [im["endpoint_indices"], im["selector_indices"], im["alpha_endpoint_indices"],
                                                                                            im["alpha_selector_indices"]], nbx, nby, alpha)
                else:
                    words = _uastc_words(src, nbx, nby, alpha)
                out = _run(program, tmp_path, codec, words)
                assert out[-1] == 0 and (out[:-1].view(np.uint8).reshape(-1, 8) == arrays[key + "_" + short]).all(), (key, short)
    rng = np.random.default_rng(99)
    for nbx, nby in ((1, 1), (1, 8), (8, 1), (2, 2), (4, 16), (16, 4), (16, 16), (64, 32)):
        n = nbx * nby
        ep = rng.integers(0, 32, (40, 4)).astype(np.uint8)
        ep[:, 3] = rng.integers(0, 8, 40)
        sel = rng.integers(0, 2 ** 32, 50, dtype=np.uint64).astype(np.uint32)
        sel[:4] = [0, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF]
        idx = [rng.integers(0, 40, n), rng.integers(0, 50, n), rng.integers(0, 40, n), rng.integers(0, 50, n)]
        if n >= 4:   # planted: an endpoint index equal to the palette's size, and a selector index far past it
            idx[0][n // 3] = 40
            idx[3][n - 1] = 65535
        for target in (P.RGB, P.RGBA):
            want, invalid = P.etc1s_state_blocks(ep, sel, idx[0], idx[1], idx[2], idx[3], nbx, nby, target)
            out = _run(program, tmp_path, "etc1s", _etc1s_words(ep, sel, idx, nbx, nby, target == P.RGBA))
            assert out[-1] == invalid == (0 if n < 4 else (2 if target == P.RGBA else 1)) and (out[:-1].view(np.uint8).reshape(-1, 8) == want).all(), (nbx, nby, target)
        blocks = rng.integers(0, 256, (n, 16)).astype(np.uint8)   # random bits: a few per cent do not unpack
        if n >= 4:
            blocks[1] = 0
            blocks[1, 0] = RESERVED_MODE_BYTE
        for target in (P.RGB, P.RGBA):
            want, invalid = P.uastc_blocks(blocks, nbx, nby, target)
            out = _run(program, tmp_path, "uastc", _uastc_words(blocks, nbx, nby, target == P.RGBA))
            assert out[-1] == invalid and (n < 4 or invalid >= 1) and (out[:-1].view(np.uint8).reshape(-1, 8) == want).all(), (nbx, nby, target)


def test_layout_sizes_offsets_and_rounding():
    images = [{"level": 0, "layer": 0, "face": 0, "num_blocks_x": 4, "num_blocks_y": 2, "width": 16, "height": 8},
              {"level": 1, "layer": 0, "face": 0, "num_blocks_x": 2, "num_blocks_y": 1, "width": 8, "height": 4},
              {"level": 2, "layer": 0, "face": 0, "num_blocks_x": 1, "num_blocks_y": 1, "width": 4, "height": 2},
              {"level": 3, "layer": 0, "face": 0, "num_blocks_x": 1, "num_blocks_y": 1, "width": 2, "height": 1}]
    lay, total = T.pvrtc1_layout(images)
    assert [(e["offset"], e["nbytes"], e["shape"], e["dtype"]) for e in lay] == [(0, 64, (8, 8), np.uint8), (64, 16, (2, 8), np.uint8), (80, 8, (1, 8), np.uint8),
                                                                                 (96, 8, (1, 8), np.uint8)] and total == 112
    assert T.PVRTC1_BYTES_PER_BLOCK == 8 and (T.PVRTC1_4_RGB, T.PVRTC1_4_RGBA) == (8, 9)
    with pytest.raises(ValueError, match="level 0, layer 0, face 0: 12 x 8 pixels: PVRTC1 only supports power of 2 dimensions"):
        T.pvrtc1_layout([dict(images[0], width=12)])


def test_refusals_come_before_the_context():
    """a target other than 8 or 9, and an image or a file that is not a power of two each way, raise by name before the device is touched"""
    arrays, _ = P.golden()
    ctx, one = M.Untouchable(), np.zeros((1, 16), np.uint8)
    etc1s, uastc = arrays["file_etc1s_opaque_basis"], arrays["file_uastc_opaque_ktx2"]
    dec = T.decode_etc1s_file(etc1s)
    for target, name in ((0, "ETC1_RGB"), (2, "BC1_RGB"), (7, "BC7_ALT"), (10, "ASTC_4x4_RGBA"), (13, "RGBA32"), (18, "PVRTC2_4_RGB"), (19, "PVRTC2_4_RGBA"), (22, "unknown")):
        for call in (lambda: T.transcode_uastc_pvrtc1_blocks(ctx, one, 1, 1, target), lambda: T.transcode_uastc_pvrtc1_file(ctx, uastc, target),
                     lambda: T.transcode_etc1s_pvrtc1_image(ctx, dec, dec["images"][0], target), lambda: T.transcode_etc1s_pvrtc1(ctx, etc1s, target),
                     lambda: T.transcode_pvrtc1_images(ctx, etc1s, target), lambda: T.transcode_pvrtc1_images(ctx, uastc, target)):
            with pytest.raises(ValueError, match=rf"PVRTC1 target {target} \({name}\) is not supported \(supported: \[8, 9\]\)"):
                call()
    with pytest.raises(ValueError, match="transcode_uastc_pvrtc1_blocks: 12 x 4 pixels: PVRTC1 only supports power of 2 dimensions"):
        T.transcode_uastc_pvrtc1_blocks(ctx, np.zeros((3, 16), np.uint8), 3, 1, 8)
    with pytest.raises(ValueError, match="transcode_etc1s_pvrtc1_image: 20 x 28 pixels: PVRTC1 only supports power of 2 dimensions"):
        T.transcode_etc1s_pvrtc1_image(ctx, dec, dict(dec["images"][0], width=20, height=28, num_blocks_x=5, num_blocks_y=7), 9)
    # files whose level 0 is not a power of two: the other transcode fixtures hold them
    odd_etc1s = np.load(ROOT / "tests" / "golden" / "etc1s_transcode_vectors.npz")["file_mip_basis"]
    for call in (lambda: T.transcode_etc1s_pvrtc1(ctx, odd_etc1s, 8), lambda: T.transcode_pvrtc1_images(ctx, odd_etc1s, 9)):
        with pytest.raises(ValueError, match="20 x 28 pixels: PVRTC1 only supports power of 2 dimensions"):
            call()
    from basis_universal_amd.backend import uastc_ktx2_file
    odd_uastc = uastc_ktx2_file(np.zeros((6, 16), np.uint8), [(0, 3, 2, 12, 8, 0, 0, 1)], srgb=False, has_alpha=True).tobytes()
    for call in (lambda: T.transcode_uastc_pvrtc1_file(ctx, odd_uastc, 8), lambda: T.transcode_pvrtc1_images(ctx, odd_uastc, 9)):
        with pytest.raises(ValueError, match="12 x 8 pixels: PVRTC1 only supports power of 2 dimensions"):
            call()
