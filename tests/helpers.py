"""Shared test plumbing: the CPU checkers (loaded and bound by native_libs.py) behind numpy-level calls, and the synthetic inputs.

Nothing here touches the product; see basis_universal_amd/ for that. The two checkers are
  * oracle/liboracle_etc1s.so   -- our plain-C restatement (travels to the GPU box as source + .so)
  * oracle/_ref/libref_harness.so -- the REAL reference compiled from /root/reference (prebuilt; travels as a binary)
"""
import ctypes as C
import functools
import pathlib

import numpy as np

import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
REF_DIR = pathlib.Path("/root/reference")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)


def ptr(a, t=u8p):
    return a.ctypes.data_as(t) if a is not None else None


# ----------------------------------------------------------------------------- inputs

def synth(w, h, seed):
    """SURVEY.md §8(d) synthetic RGBA image: smooth sinusoids + 4x4 tile noise N(0,12) + pixel noise N(0,6)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 3), np.float32)
    img[..., 0] = 128 + 100 * np.sin(x / 97) * np.cos(y / 131)
    img[..., 1] = 128 + 90 * np.sin((x + y) / 211)
    img[..., 2] = 128 + 110 * np.cos(x / 53 + y / 71)
    tile = rng.normal(0, 12, (h // 4, w // 4, 3)).astype(np.float32)
    img += np.repeat(np.repeat(tile, 4, axis=0), 4, axis=1)
    img += rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = np.clip(img, 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def uniform_random(w, h, seed=42):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    out[..., 3] = 255
    return out


def endpoint_cube(w, h, seed=7):
    """The worst case for the ENDPOINT codebook builder: block b is drawn from the four colours of ETC1S endpoint (colour5, intensity table) number perm[b mod 2^18] with
    random selectors, so the per-block fit finds (nearly) every one of the 32^3 x 8 endpoints and the builder gets as many distinct training vectors as an image can give it
    (236,235 is the ceiling, tests/test_host_logic.py::test_endpoint_codebook_can_never_reach_the_threaded_gate; 14,177 for uniform noise, 35,502 for the synthetic image)."""
    rng = np.random.default_rng(seed)
    nb = (h // 4) * (w // 4)
    code = rng.permutation(1 << 18)[np.arange(nb) % (1 << 18)]
    table = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106], [-183, -47, 47, 183]], np.int32)
    c5 = np.stack([(code >> 10) & 31, (code >> 5) & 31, code & 31], -1).astype(np.int32)
    c8 = (c5 << 3) | (c5 >> 2)
    sel = rng.integers(0, 4, (nb, 16))
    d = table[(code >> 15) & 7][np.arange(nb)[:, None], sel]                       # (nb, 16)
    px = np.clip(c8[:, None, :] + d[:, :, None], 0, 255).astype(np.uint8)          # (nb, 16, 3)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 3] = 255
    out[..., :3] = px.reshape(h // 4, w // 4, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, 3)
    return out


def kodak_mosaic(w=4096, h=4096):
    """The 24 Kodak images of the reference's own test set (tests/golden/kodak24.npz: the pixels of test_files/kodim01-24.png) tiled into one w x h RGBA image:
    photographic statistics at BASELINE.json's full size. 768 x 512 slots, portrait images transposed; slot i holds image i mod 24, mirrored top to bottom from
    the second time round (so no block repeats); cropped to w x h."""
    z = np.load(pathlib.Path(__file__).parent / "golden" / "kodak24.npz")
    imgs = [z[f"k{i:02d}"] for i in range(1, 25)]
    imgs = [im if im.shape[0] == 512 else np.ascontiguousarray(im.transpose(1, 0, 2)) for im in imgs]
    cols, rows = (w + 767) // 768, (h + 511) // 512
    out = np.empty((rows * 512, cols * 768, 4), np.uint8)
    out[..., 3] = 255
    for i in range(rows * cols):
        im = imgs[i % 24]
        if (i // 24) & 1:
            im = im[::-1]
        r, c = divmod(i, cols)
        out[r * 512:(r + 1) * 512, c * 768:(c + 1) * 768, :3] = im
    return np.ascontiguousarray(out[:h, :w])


def to_pixel_blocks(img):
    """(H, W, 4) u8 -> (n_blocks, 4, 4, 4) u8 in block-raster order, [y][x] inside the block (comp.cpp:3207-3268).
    Edges are clamped like image::extract_block_clamped."""
    h, w, _ = img.shape
    bh, bw = (h + 3) // 4, (w + 3) // 4
    if (h % 4) or (w % 4):
        ys = np.minimum(np.arange(bh * 4), h - 1)
        xs = np.minimum(np.arange(bw * 4), w - 1)
        img = img[ys][:, xs]
    blocks = img.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(blocks.reshape(bh * bw, 4, 4, 4))


def load_png(path):
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGBA"), dtype=np.uint8))


def csr_from_lists(lists):
    offs = np.zeros(len(lists) + 1, np.uint32)
    offs[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if len(lists) and offs[-1] else np.zeros(0, np.uint32)
    return offs, np.ascontiguousarray(idx, np.uint32)


def csr_blob_split(blob):
    """[n, off_0..off_n, idx...] u32 blob (oracle/ref_harness.cpp csr()) -> (offsets, indices)."""
    n = int(blob[0])
    offs = blob[1:n + 2].copy()
    idx = blob[n + 2:n + 2 + int(offs[-1])].copy()
    return offs, idx


# ----------------------------------------------------------------------------- C oracle

def oracle():
    return native_libs.load("oracle")


def orc_encode_blocks(blocks, level, perceptual=True):
    n = blocks.shape[0]
    out = np.zeros((n, 8), np.uint8)
    oracle().orc_encode_etc1s_blocks(ptr(blocks), n, level, int(perceptual), ptr(out))
    return out


def etc1s_test_tiles():
    """The ~3,500 tiles of the ETC1S kernel parity tests: a synthetic image, uniform noise, flat tiles (white, black, one dark red run) and a two-channel gradient."""
    a = to_pixel_blocks(synth(256, 192, 1234))
    b = to_pixel_blocks(uniform_random(64, 64, 42))
    flat = np.zeros((64, 4, 4, 4), np.uint8)
    flat[:, :, :, 3] = 255
    flat[:32, :, :, :3] = 255
    flat[40:48, :, :, 0] = 17
    grad = np.zeros((32, 64, 4), np.uint8)
    grad[..., 0] = np.arange(64)[None, :] * 4
    grad[..., 1] = np.arange(32)[:, None] * 8
    grad[..., 3] = 255
    return np.concatenate([a, b, flat, to_pixel_blocks(grad)])


ETC1_INTEN_TABLES = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106],
                              [-183, -47, 47, 183]], np.int32)
PLANT_CLASSES = ("inside", "low", "high", "both", "split")
PLANT_TILES_PER_ENDPOINT = 12
PLANT_NOISE = (0, 0, 1, 3)


def etc1s_clamp_class(color5, table):
    """How the outer colours of ETC1S endpoints (color5 (..., 3), table (...)) clamp: 0 = neither base - b nor base + b leaves 0..255 in any channel, 1 = only base - b
    does (low), 2 = only base + b does (high), 3 = both do."""
    c5 = np.asarray(color5, np.int32)
    c8 = (c5 << 3) | (c5 >> 2)
    b = ETC1_INTEN_TABLES[np.asarray(table, np.int64), 3]
    return ((c8.min(axis=-1) - b < 0) * 1 + (c8.max(axis=-1) + b > 255) * 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _planted_tiles():
    rng = np.random.default_rng(20241)
    all5 = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    all8 = (all5 << 3) | (all5 >> 2)
    mn, mx = all8.min(axis=1), all8.max(axis=1)
    tiles, meta = [], []
    endpoint = 0
    for t in range(8):
        b = int(ETC1_INTEN_TABLES[t, 3])
        lo, hi = mn - b < 0, mx + b > 255
        member = {"inside": ~lo & ~hi, "low": lo & ~hi, "high": ~lo & hi, "both": lo & hi & (mx - mn < 60), "split": lo & hi & (mx - mn >= 120)}
        for ci, cls in enumerate(PLANT_CLASSES):
            if not member[cls].any():   # no base of table 7 stays inside; only tables 6 and 7 clamp at both ends with channels that close
                continue
            picked = set()
            while len(picked) < 6:      # rejection: draw colour5 values until six distinct members of the class have come up
                c = int(rng.integers(0, 1 << 15))
                if member[cls][c]:
                    picked.add(c)
            for c in sorted(picked):
                for k in range(PLANT_TILES_PER_ENDPOINT):
                    sel = rng.integers(0, 4, 16)
                    sel[:4] = rng.permutation(4)
                    a = PLANT_NOISE[k % len(PLANT_NOISE)]
                    clean = np.clip(all8[c][None, :] + ETC1_INTEN_TABLES[t][sel][:, None], 0, 255)
                    px = np.clip(clean + rng.integers(-a, a + 1, (16, 3)), 0, 255)
                    tile = np.full((16, 4), 255, np.uint8)
                    tile[:, :3] = px
                    tiles.append(tile.reshape(4, 4, 4))
                    meta.append((t, ci, endpoint, a, tuple(int(v) for v in all5[c])))
                endpoint += 1
    meta = np.array(meta, np.dtype([("table", np.uint8), ("cls", np.uint8), ("endpoint", np.uint32), ("noise", np.uint8), ("color5", np.uint8, 3)]))
    tiles = np.ascontiguousarray(np.stack(tiles))
    tiles.setflags(write=False); meta.setflags(write=False)
    return tiles, meta


def etc1s_planted_tiles():
    """-> (tiles (n, 4, 4, 4) u8, meta): tiles drawn from the four colours of a PLANTED ETC1S endpoint, so that every intensity table wins somewhere and the winning
    endpoint's outer colours clamp in every way they can. Per table 0..7 and per clamp class (PLANT_CLASSES; mn, mx the smallest and largest channel of the scaled base, b the
    table's outer step: inside = nothing clamps, low = only mn - b < 0, high = only mx + b > 255, both = both with mx - mn < 60, split = both with mx - mn >= 120, one channel
    clamping low while another clamps high) six base colours found by rejection, classes no base of the table falls in left out; per endpoint twelve tiles of sixteen random
    selectors, the first four a permutation of 0..3, texel = clamp(base + delta[selector]) plus uniform noise of amplitude 0, 0, 1, 3 (in turn), clamped again. Alpha is 255.
    meta (structured, one record per tile): table, cls (index into PLANT_CLASSES), endpoint (0.., ordered by table, then class), noise, color5. Read-only, seeded."""
    return _planted_tiles()


@functools.lru_cache(maxsize=None)
def etc1s_spread_ladder():
    """768 tiles: for every spread s in 0..255 and every channel c one tile whose channel c spans exactly [l0, l0 + s], both extremes present, the other two channels
    spanning at most s -- the block's (and, as a cluster of its two sub-blocks, the cluster's) index into the per-spread intensity table mask is s. Read-only, seeded."""
    rng = np.random.default_rng(20242)
    tiles = np.full((768, 16, 4), 255, np.uint8)
    for s in range(256):
        for c in range(3):
            t = tiles[s * 3 + c]
            for ch in range(3):
                span = s if ch == c else int(rng.integers(0, s + 1))
                l0 = int(rng.integers(0, 256 - span))
                t[:, ch] = rng.integers(l0, l0 + span + 1, 16)
                if ch == c:
                    where = rng.permutation(16)[:2]
                    t[where[0], ch], t[where[1], ch] = l0, l0 + s
    tiles = np.ascontiguousarray(tiles.reshape(768, 4, 4, 4))
    tiles.setflags(write=False)
    return tiles


def etc1s_planted_test_tiles():
    """The second tile set of the ETC1S kernel parity tests: the planted tiles followed by the spread ladder."""
    return np.ascontiguousarray(np.concatenate([etc1s_planted_tiles()[0], etc1s_spread_ladder()]))


def clusters_by_plant(meta):
    """The endpoint clustering the planted tiles were made for, in clusters_by_luma's shape: cluster e = both sub-blocks of every tile of planted endpoint e."""
    ep = np.asarray(meta["endpoint"], np.uint32)
    lists = []
    for e in range(int(ep.max()) + 1):
        run = np.nonzero(ep == e)[0]
        lists.append(np.stack([run * 2, run * 2 + 1], axis=1).reshape(-1).astype(np.uint32))
    return lists, ep.copy()


def planted_exact_clusters(meta, count=24):
    """`count` clusters the cluster fit can reproduce exactly: the first two noise-free tiles of one planted endpoint each, endpoints spread evenly over the tables and clamp
    classes (the clusters of clusters_by_plant hold the noisy tiles too, and none of them comes out with error 0)."""
    n_ep = int(meta["endpoint"].max()) + 1
    lists = []
    for e in np.linspace(0, n_ep - 1, count).astype(np.int64):
        run = np.nonzero((meta["endpoint"] == e) & (meta["noise"] == 0))[0][:2]
        lists.append(np.stack([run * 2, run * 2 + 1], axis=1).reshape(-1).astype(np.uint32))
    return lists


def planted_endpoint_codebook(perceptual=1, level=1):
    """-> fresh copies of (the oracle's fit of clusters_by_plant's clusters, about 200 x {r5, g5, b5, inten} with every table and clamp class present, the cluster of every tile of
    etc1s_planted_test_tiles: its planted endpoint, and for a ladder tile the cluster whose colour5 is nearest to the tile's mean colour)"""
    params, block_cluster = _planted_endpoint_codebook(int(perceptual), level)
    return params.copy(), block_cluster.copy()


@functools.lru_cache(maxsize=None)
def _planted_endpoint_codebook(perceptual, level):
    tiles, meta = etc1s_planted_tiles()
    blocks = etc1s_planted_test_tiles()
    lists, block_cluster = clusters_by_plant(meta)
    k = len(lists)
    offs, idx = csr_from_lists(lists)
    params = np.zeros((k, 4), np.uint8); err = np.zeros(k, np.uint64); valid = np.zeros(k, np.uint8)
    oracle().orc_generate_endpoint_codebook(ptr(blocks), k, ptr(offs, u32p), ptr(idx, u32p), level, perceptual, 0, ptr(params), ptr(err, u64p), ptr(valid))
    assert valid.all()
    ladder = blocks[tiles.shape[0]:, :, :, :3].reshape(-1, 16, 3).astype(np.float64).mean(axis=1)
    base = ((params[:, :3].astype(np.int32) << 3) | (params[:, :3] >> 2)).astype(np.float64)
    near = ((ladder[:, None, :] - base[None, :, :]) ** 2).sum(axis=2).argmin(axis=1).astype(np.uint32)
    return params, np.ascontiguousarray(np.concatenate([block_cluster, near]))


def clusters_by_luma(blocks, k, rng):
    """A plausible endpoint clustering: blocks sorted by mean luma cut into k uneven runs; both subblocks stay together."""
    n = blocks.shape[0]
    order = np.argsort(blocks[..., :3].reshape(n, -1).astype(np.int64).sum(axis=1), kind="stable")
    cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False))
    lists, block_cluster = [], np.zeros(n, np.uint32)
    for ci, run in enumerate(np.split(order, cuts)):
        run = rng.permutation(run)
        lists.append(np.stack([run * 2, run * 2 + 1], axis=1).reshape(-1).astype(np.uint32))
        block_cluster[run] = ci
    return lists, block_cluster


def endpoint_codebook(blocks, k, seed, level=1, perceptual=1):
    """-> (k x {r5, g5, b5, inten} of the oracle's fit of clusters_by_luma's clusters, the cluster of every block)"""
    rng = np.random.default_rng(seed)
    lists, block_cluster = clusters_by_luma(blocks, k, rng)
    offs, idx = csr_from_lists(lists)
    params = np.zeros((k, 4), np.uint8); err = np.zeros(k, np.uint64); valid = np.zeros(k, np.uint8)
    oracle().orc_generate_endpoint_codebook(ptr(blocks), k, ptr(offs, u32p), ptr(idx, u32p), level, perceptual, 0, ptr(params), ptr(err, u64p), ptr(valid))
    return params, block_cluster


# ----------------------------------------------------------------------------- the real reference

def have_ref():
    return (ORACLE_DIR / "_ref" / "libref_harness.so").exists()


def ref_harness_version():
    """ref_harness_version() of oracle/_ref/libref_harness.so: 0 = no harness, 1 = a build from before the function existed (an oracle/_ref/ carried over from an
    earlier revision where the reference is not there to rebuild it: oracle/Makefile rebuilds it wherever it is), else what the harness says (oracle/ref_harness.cpp)."""
    if not have_ref():
        return 0
    L = ref()
    if not hasattr(L, "ref_harness_version"):
        return 1
    return int(L.ref_harness_version())


@functools.lru_cache(maxsize=None)
def ref():
    L = native_libs.load("ref")
    assert L.ref_init() == 1
    return L


def ref_quality_effort(uastc, quality, effort):
    """basis_compressor_params::set_format_mode_and_quality_effort of the reference -> (etc1s quality, etc1s comp level, uastc pack flags, rdo flag, lambda as f32)"""
    out, lam = np.zeros(4, np.int32), np.zeros(1, np.float32)
    assert ref().ref_quality_effort(int(uastc), quality, effort, out.ctypes.data_as(C.POINTER(C.c_int32)), ptr(lam, f32p)) == 1
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3]), lam[0]


class RefFrontend:
    """The reference's basisu_frontend, driven one private stage at a time (oracle/ref_harness.cpp)."""

    def __init__(self, blocks, max_ep, max_sel, level, perceptual=True, threads=1):
        """threads: the reference's job pool size including the caller; 1 is the pinned configuration every parity check uses"""
        self.L = ref()
        self.blocks = np.ascontiguousarray(blocks)
        if threads == 1:
            self.h = self.L.ref_frontend_create(ptr(self.blocks), self.blocks.shape[0], max_ep, max_sel, level, int(perceptual))
        else:
            self.h = self.L.ref_frontend_create_mt(ptr(self.blocks), self.blocks.shape[0], max_ep, max_sel, level, int(perceptual), threads)
        assert self.h

    def call(self, name, arg=0):
        r = self.L.ref_frontend_call(self.h, name.encode(), arg)
        assert r != -1, name
        return r

    def get(self, name, dtype=np.uint8):
        need = self.L.ref_frontend_get(self.h, name.encode(), None, 0)
        assert need != 2 ** 64 - 1, name
        buf = np.zeros(need, np.uint8)
        self.L.ref_frontend_get(self.h, name.encode(), buf.ctypes.data_as(C.c_void_p), need)
        return buf.view(dtype)

    def get_csr(self, name):
        return csr_blob_split(self.get(name, np.uint32))

    def backend_encoder_blocks(self, nbx, nby, endpoint_thresh=1.5, selector_thresh=1.25):
        """basisu_backend::create_encoder_blocks on the finished frontend (2D, one slice). Returns a dict of arrays + the CPU seconds."""
        n = nbx * nby
        ep, pred, sel = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
        k_ep = int(self.get("endpoint_cluster_etc_params").size // 1) if False else 65536
        o2n, n2o = np.full(k_ep, 0xFFFFFFFF, np.uint32), np.full(k_ep, 0xFFFFFFFF, np.uint32)
        secs = C.c_double(0)
        f = self.L.ref_backend_create_encoder_blocks
        assert f(self.h, nbx, nby, endpoint_thresh, selector_thresh, ep.ctypes.data, pred.ctypes.data, sel.ctypes.data, o2n.ctypes.data, n2o.ctypes.data, C.byref(secs)) == 1
        return {"endpoint_index": ep, "predictor": pred, "selector_index": sel, "endpoint_old_to_new": o2n[o2n != 0xFFFFFFFF],
                "selector_new_to_old": n2o[n2o != 0xFFFFFFFF], "seconds": secs.value}

    def backend_run(self, slices, endpoint_thresh=1.5, selector_thresh=1.25):
        """basisu_backend::encode on the finished frontend; slices = [(first_block, nbx, nby), ...]. Returns (bytes, seconds)."""
        sl = np.ascontiguousarray(np.asarray(slices, np.uint32).reshape(-1, 3))
        secs = C.c_double(0)
        n = self.L.ref_backend_run(self.h, sl.ctypes.data_as(C.c_void_p), sl.shape[0], endpoint_thresh, selector_thresh, C.byref(secs))
        return n, secs.value

    def backend_get(self, name, slice_index=0, dtype=np.uint8):
        need = self.L.ref_backend_get(self.h, name.encode(), slice_index, None, 0)
        assert need != 2 ** 64 - 1, name
        buf = np.zeros(need, np.uint8)
        self.L.ref_backend_get(self.h, name.encode(), slice_index, buf.ctypes.data_as(C.c_void_p), need)
        return buf.view(dtype)

    def set_tex_type(self, tex_type):
        """basist::basis_texture_type of the frontend params (3 = video frames); before compress."""
        self.L.ref_frontend_set_tex_type(self.h, tex_type)

    def set_state(self, color5_inten, selectors16, block_endpoint, block_selector):
        """Overwrite the finished frontend state with arbitrary codebooks / assignments (backend fuzzing)."""
        f = self.L.ref_frontend_set_state
        ep = np.ascontiguousarray(color5_inten, np.uint8).reshape(-1, 4)
        sel = np.ascontiguousarray(selectors16, np.uint8).reshape(-1, 16)
        be, bs = np.ascontiguousarray(block_endpoint, np.uint32), np.ascontiguousarray(block_selector, np.uint32)
        assert f(self.h, ep.shape[0], ep.ctypes.data, sel.shape[0], sel.ctypes.data, be.ctypes.data, bs.ctypes.data) == 1

    def reoptimize(self, new_block_endpoints, final_codebook, block_selector_indices=None):
        """basisu_frontend::reoptimize_remapped_endpoints on this frontend -> old_to_new (int32, one per endpoint cluster before the call)."""
        f = self.L.ref_frontend_reoptimize
        nb = np.ascontiguousarray(new_block_endpoints, np.uint32)
        k = self.get("endpoint_cluster_etc_params").size // 16
        o2n = np.full(max(k, 1), -1, np.int32)
        sel = None if block_selector_indices is None else np.ascontiguousarray(block_selector_indices, np.uint32)
        assert f(self.h, nb.ctypes.data, nb.size, o2n.ctypes.data, int(final_codebook), None if sel is None else sel.ctypes.data) == 1
        return o2n

    def basis_file(self, tex_type=0, userdata0=0, userdata1=0, y_flipped=False, us_per_frame=0, key_values=()):
        """basisu_file::init on the last backend_run's output -> the .basis file bytes."""
        f = self.L.ref_basis_file
        n = len(key_values)
        keys = (C.c_char_p * max(n, 1))(*[k.encode() for k, _ in key_values])
        bufs = [np.frombuffer(bytes(v), np.uint8) if len(v) else np.zeros(1, np.uint8) for _, v in key_values]
        vals = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        sizes = np.array([len(v) for _, v in key_values] + [0], np.uint32)
        args = (self.h, tex_type, userdata0, userdata1, int(y_flipped), us_per_frame, keys, vals, sizes.ctypes.data, n)
        need = f(*args, None, 0)
        assert need, "ref_basis_file failed"
        out = np.zeros(need, np.uint8)
        f(*args, out.ctypes.data, need)
        return out

    def close(self):
        if self.h:
            self.L.ref_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


# ----------------------------------------------------------------------------- UASTC

def uastc_test_blocks():
    """~1.2k source blocks covering every class encode_uastc distinguishes (uastc_enc.cpp:3135-3152) plus degenerate cases."""
    rng = np.random.default_rng(77)
    parts = [to_pixel_blocks(synth(64, 64, 1234)), to_pixel_blocks(uniform_random(32, 32, 42))]
    parts.append(to_pixel_blocks(np.load(ROOT / "tests" / "golden" / "kodim03.npz")["rgba"][200:264, 300:364]))   # the reference's test_files/kodim03.png
    g = synth(48, 48, 5).copy(); g[..., 1] = g[..., 0]; g[..., 2] = g[..., 0]
    parts.append(to_pixel_blocks(g))
    yy, xx = np.mgrid[0:48, 0:48]
    a = synth(48, 48, 11).copy(); a[..., 3] = np.clip(128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 0, 255).astype(np.uint8)
    parts.append(to_pixel_blocks(a))
    an = synth(32, 32, 9).copy(); an[..., 3] = rng.integers(0, 256, (32, 32), dtype=np.uint8)
    parts.append(to_pixel_blocks(an))
    ga = g.copy(); ga[..., 3] = a[..., 3]
    parts.append(to_pixel_blocks(ga))
    parts.append(np.ascontiguousarray(rng.integers(0, 256, (48, 1, 1, 4), dtype=np.uint8).repeat(4, 1).repeat(4, 2)))  # solid, any alpha
    two = rng.integers(0, 256, (96, 2, 4), dtype=np.uint8)
    tb = two[np.arange(96)[:, None], rng.integers(0, 2, (96, 16))].reshape(96, 4, 4, 4)
    tb[:64, :, :, 3] = 255
    parts.append(np.ascontiguousarray(tb))
    ramp = np.zeros((32, 4, 4, 4), np.uint8)  # one-channel ramps and near-solid blocks (degenerate endpoint handling)
    for i in range(32):
        ramp[i, :, :, :3] = rng.integers(0, 256, 3)
        ramp[i, :, :, i % 3] = (np.arange(16).reshape(4, 4) * (1 + i % 5) + i) % 256
        ramp[i, :, :, 3] = 255
    parts.append(ramp)
    # piecewise blocks: 2 or 3 regions with unrelated colour (and alpha) ramps, so the multi-subset modes (2, 3, 4, 7, 9, 16) win somewhere
    yy4, xx4 = np.mgrid[0:4, 0:4]
    masks = [xx4 >= 2, yy4 >= 2, xx4 + yy4 >= 4, xx4 >= 1, yy4 >= 3, xx4 > yy4, (xx4 >= 1) + (xx4 >= 3), (yy4 >= 1) + (yy4 >= 2) * 1, (xx4 + yy4 >= 2) * 1 + (xx4 + yy4 >= 5)]
    pw = np.zeros((len(masks) * 24, 4, 4, 4), np.uint8)
    for i in range(pw.shape[0]):
        m = masks[i % len(masks)].astype(np.int64)
        variant = i // len(masks)
        for region in range(int(m.max()) + 1):
            base = rng.integers(0, 256, 4)
            slope = rng.integers(-12, 13, (2, 4))
            v = base + xx4[..., None] * slope[0] + yy4[..., None] * slope[1] + rng.integers(-2, 3, (4, 4, 4))
            pw[i][m == region] = np.clip(v, 0, 255).astype(np.uint8)[m == region]
        if variant % 3 == 0:
            pw[i, :, :, 3] = 255
        elif variant % 3 == 1:
            pw[i, :, :, 1] = pw[i, :, :, 0]; pw[i, :, :, 2] = pw[i, :, :, 0]  # luminance + alpha
    parts.append(pw)
    return np.ascontiguousarray(np.concatenate(parts))


def uastc_flag_sets():
    """(name, pack flags): every level plus each option flag (uastc_enc.h:24-66) on top of the default level."""
    sets = [(f"level{l}", l) for l in range(5)]
    sets += [("favor_uastc", 2 | 8), ("favor_bc7", 2 | 16), ("etc1_faster", 2 | 64), ("etc1_fastest", 2 | 128),
             ("etc1_noflip", 2 | 256), ("favor_simpler", 2 | 512), ("level1_faster_simpler", 1 | 64 | 512), ("level3_favor_bc7", 3 | 16)]
    return sets


def ref_encode_uastc(blocks, flags):
    blocks = np.ascontiguousarray(blocks)
    n = blocks.shape[0]
    out = np.zeros((n, 16), np.uint8)
    ref().ref_encode_uastc(ptr(blocks), n, flags, ptr(out))
    return out


RDO_DEFAULTS = dict(lam=1.0, max_rms_ratio=10.0, skip_rms=8.0, smooth_std_dev=18.0, smooth_scale=10.0, dict_size=4096, literal_cost=100, refine=1)


def rdo_param_arrays(**kw):
    """uastc_rdo_params (uastc_enc.h:94-134) as the (float[5], uint32[3]) pair the harnesses take."""
    p = dict(RDO_DEFAULTS)
    p.update(kw)
    return (np.array([p["lam"], p["max_rms_ratio"], p["skip_rms"], p["smooth_std_dev"], p["smooth_scale"]], np.float32),
            np.array([p["dict_size"], p["literal_cost"], p["refine"]], np.uint32))


def uastc_rdo_cases():
    """(name, pack flags, total_jobs, uastc_rdo_params overrides) of the committed RDO known answers (tests/golden/uastc_rdo_vectors.npz)."""
    return [("default_l2", 2, 0, dict(lam=1.0)),
            ("jobs4_l2", 2, 4, dict(lam=1.0)),
            ("strong_l2", 2, 0, dict(lam=4.0)),
            ("norefine_l0", 0, 3, dict(lam=3.0, refine=0)),
            ("bigdict_l1", 1, 0, dict(lam=2.0, dict_size=32768)),
            ("tinydict_l2", 2, 5, dict(lam=10.0, dict_size=64, skip_rms=30.0)),
            ("settle_l0", 0, 0, dict(lam=20.0)),
            ("tuned_l3", 3, 2, dict(lam=1.5, max_rms_ratio=1.5, smooth_std_dev=40.0, smooth_scale=3.0, literal_cost=150))]


def synth_smooth(w, h, seed):
    """Low-noise RGBA image: blocks that UASTC encodes in mode 0 and that RDO modifies and refits a lot."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 4), np.float32)
    img[..., 0] = 128 + 100 * np.sin(x / 17) * np.cos(y / 23)
    img[..., 1] = 128 + 90 * np.sin(x / 29 + 1) * np.cos(y / 13)
    img[..., 2] = 128 + 80 * np.cos(x / 11) * np.sin(y / 19 + 2)
    img[..., 3] = 255
    img[..., :3] += rng.normal(0, 2.0, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def smooth_with_la_blocks(w, h, seed):
    """synth_smooth as blocks, every 4th block luminance+alpha: modes 15/17 next to modified mode-0 blocks, the one arrangement in which
    the selector field of a block overlaps the (refitted) endpoint bits of its neighbours (uastc_rdo.h, deferred write-back)."""
    b = to_pixel_blocks(synth_smooth(w, h, seed)).copy()
    grey = b[::4, :, :, 1].copy()
    b[::4, :, :, 0] = grey
    b[::4, :, :, 2] = grey
    b[::4, :, :, 3] = 255 - grey // 2
    return b


def uastc_rdo_test_blocks():
    """Source blocks of the RDO vectors: a smooth+noise image (neighbouring blocks resemble each other, which is what RDO feeds on), part
    of it with a smooth alpha channel, followed by the every-class block set of the encoder vectors."""
    b = to_pixel_blocks(synth(256, 96, 11)).copy()
    b[1024:, :, :, 3] = b[1024:, :, :, 0] // 2 + 60
    return np.ascontiguousarray(np.concatenate([b, smooth_with_la_blocks(192, 64, 3), uastc_test_blocks()[::3]]))


def ref_uastc_rdo(packed, blocks, flags, total_jobs=0, **kw):
    fp, up = rdo_param_arrays(**kw)
    out = np.ascontiguousarray(packed).copy()
    blocks = np.ascontiguousarray(blocks)
    assert ref().ref_uastc_rdo(ptr(out), ptr(blocks), out.shape[0], ptr(fp, f32p), ptr(up, u32p), flags, total_jobs) == 1
    return out


def host_uastc_rdo(packed, blocks, flags, total_jobs=0, table_trials=False, **kw):
    """The host build of uastc_rdo.h under a scalar strip loop; table_trials scores trials from the per-block error table like the GPU kernel."""
    fp, up = rdo_param_arrays(**kw)
    total_jobs |= 0x80000000 if table_trials else 0
    out = np.ascontiguousarray(packed).copy()
    blocks = np.ascontiguousarray(blocks)
    assert uastc_host().hc_uastc_rdo(ptr(out), ptr(blocks), out.shape[0], ptr(fp, f32p), ptr(up, u32p), flags, total_jobs) == 1
    return out


def host_uastc_rdo_counted(packed, blocks, flags, total_jobs=0, table_trials=False, **kw):
    """host_uastc_rdo plus {"modified", "refined", "skipped"}, counted where the kernels count them (bu_hip_k_uastc_rdo's out_stats)."""
    fp, up = rdo_param_arrays(**kw)
    total_jobs |= 0x80000000 if table_trials else 0
    out = np.ascontiguousarray(packed).copy()
    blocks = np.ascontiguousarray(blocks)
    counts = np.zeros(3, np.uint32)
    assert uastc_host().hc_uastc_rdo_counted(ptr(out), ptr(blocks), out.shape[0], ptr(fp, f32p), ptr(up, u32p), flags, total_jobs, ptr(counts, u32p)) == 1
    return out, dict(modified=int(counts[0]), refined=int(counts[1]), skipped=int(counts[2]))


def uastc_host():
    """The UASTC device core compiled for the host (tests/native/uastc_host.cpp): a checker for the CPU-only suite."""
    return native_libs.load("uastc_host")


def fsum_host():
    """csrc/fsum_scan.h (the order-preserving float sum of the wide TSVQ kernels) compiled for the host: tests/native/fsum_host.cpp."""
    return native_libs.load("fsum_host")


def tt_exact_host():
    """csrc/tt_exact.h (when a block of the reference's double accumulators can be taken in one step: tsvq_wide6_kernels.hip, tt_walk) compiled for the host:
    tests/native/tt_exact_host.cpp."""
    return native_libs.load("tt_exact_host")


# the records of include/basisu_hip.h as numpy structured dtypes
TSVQ_ROOT = np.dtype([("origin", np.float32, 16), ("weight", np.uint64), ("var", np.float32), ("pad", np.uint32)])
TSVQ_NODE = np.dtype([("buf", np.uint32), ("start", np.uint32), ("count", np.uint32), ("pad", np.uint32), ("weight", np.uint64), ("origin", np.float32, 16)])
TSVQ_SPLIT = np.dtype([("ok", np.uint32), ("l_count", np.uint32), ("r_count", np.uint32), ("pad", np.uint32), ("l_weight", np.uint64), ("r_weight", np.uint64),
                       ("l_var", np.float32), ("r_var", np.float32), ("l_centroid", np.float32, 16), ("r_centroid", np.float32, 16)])
TSVQ_SPAN = np.dtype([("buf", np.uint32), ("start", np.uint32), ("count", np.uint32), ("value", np.uint32)])
assert (TSVQ_ROOT.itemsize, TSVQ_NODE.itemsize, TSVQ_SPLIT.itemsize, TSVQ_SPAN.itemsize) == (80, 88, 168, 16)


def tsvq_node_host():
    """csrc/host/tsvq.h one node at a time (tests/native/tsvq_node_host.cpp): the root record of a member list, the split record + child lists of a node."""
    return native_libs.load("tsvq_node_host")


class TsvqNodes:
    """The per-node host reference over one training set (rows (n, dim) float32, weights (n,) uint64)."""

    def __init__(self, rows, weights):
        self.L = tsvq_node_host()
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.weights = np.ascontiguousarray(weights, np.uint64)
        self.n, self.dim = self.rows.shape
        self.h = self.L.tn_open(self.dim, ptr(self.rows, f32p), ptr(self.weights, u64p), self.n)
        assert self.h

    def root(self, members):
        """-> TSVQ_ROOT scalar: make_root over `members` in list order"""
        m = np.ascontiguousarray(members, np.uint32)
        out = np.zeros(1, TSVQ_ROOT)
        self.L.tn_root(self.h, ptr(m, u32p), m.size, out.ctypes.data_as(C.c_void_p))
        return out[0]

    def split(self, members, weight, origin):
        """-> (TSVQ_SPLIT scalar with RAW variances, left list, right list); ok == 0 (and empty lists) where prep_split / refine_split return false"""
        m = np.ascontiguousarray(members, np.uint32)
        o = np.zeros(16, np.float32); o[:self.dim] = np.asarray(origin, np.float32)[:self.dim]
        out = np.zeros(1, TSVQ_SPLIT); kids = np.zeros(max(m.size, 1), np.uint32)
        self.L.tn_split(self.h, ptr(m, u32p), m.size, int(weight), ptr(o, f32p), out.ctypes.data_as(C.c_void_p), ptr(kids, u32p))
        r = out[0]
        if not r["ok"]:
            return r, kids[:0], kids[:0]
        return r, kids[:int(r["l_count"])].copy(), kids[int(r["l_count"]):m.size].copy()

    def close(self):
        if self.h:
            self.L.tn_close(self.h)
            self.h = None

    def __del__(self):
        self.close()


# the packed PODs of include/basisu_hip.h section 1 (= encoder/basisu_opencl.h) as numpy structured dtypes
BU_COLOR = np.dtype([("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("a", np.uint8)])
BU_PIXEL_CLUSTER = np.dtype([("total_pixels", np.uint64), ("first_pixel_index", np.uint64)])
BU_BLOCK_INFO = np.dtype([("first_cluster_ofs", np.uint16), ("num_clusters", np.uint16), ("cur_cluster_index", np.uint16), ("cur_cluster_etc_inten", np.uint8)])
BU_ENDPOINT_CLUSTER = np.dtype([("unscaled_color", BU_COLOR), ("etc_inten", np.uint8), ("cluster_index", np.uint16)])
BU_FOSC_SELECTOR = np.dtype([("packed_selectors", np.uint32)])
BU_FOSC_BLOCK = np.dtype([("etc_color5_inten", BU_COLOR), ("first_selector", np.uint32), ("num_selectors", np.uint32)])
assert (BU_PIXEL_CLUSTER.itemsize, BU_BLOCK_INFO.itemsize, BU_ENDPOINT_CLUSTER.itemsize, BU_FOSC_SELECTOR.itemsize, BU_FOSC_BLOCK.itemsize) == (16, 7, 7, 4, 12)


def seam_translate_host():
    """csrc/host/seam_translate.h (the host translations behind section 1 of include/basisu_hip.h) compiled for the host: tests/native/seam_translate_host.cpp."""
    return native_libs.load("seam_translate_host")


def _seam_tables(handle, err, layout):
    """-> (dict of arrays, None) for a translation that succeeded, (None, the refusal's text) otherwise"""
    L = seam_translate_host()
    if not handle:
        assert err.value, "refused without a text"
        return None, err.value.decode()
    assert err.value is None
    out = {}
    for i, (name, dtype) in enumerate(layout):
        need = L.st_get(handle, i, None, 0)
        assert need != 2 ** 64 - 1 and need % np.dtype(dtype).itemsize == 0
        buf = np.zeros(need // np.dtype(dtype).itemsize, dtype)
        L.st_get(handle, i, buf.ctypes.data_as(C.c_void_p), need)
        out[name] = buf
    L.st_free(handle)
    return out, None


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


_WINDOWS = [("cand_offsets", np.uint32), ("cand_indices", np.uint32), ("block_parent", np.uint8)]


def seam_refine_tables(info, clusters, null=()):
    """translate_refine over BU_BLOCK_INFO / BU_ENDPOINT_CLUSTER arrays; `null` names arguments handed over as NULL with their counts kept"""
    err = C.c_char_p()
    h = seam_translate_host().st_refine(None if "info" in null else _vp(info), info.size, clusters.size, None if "clusters" in null else _vp(clusters), C.byref(err))
    return _seam_tables(h, err, [("params", np.uint32)] + _WINDOWS + [("block_cur", np.uint32)])


def seam_fosc_tables(info, selectors, null=()):
    err = C.c_char_p()
    h = seam_translate_host().st_fosc(None if "info" in null else _vp(info), info.size, selectors.size, None if "selectors" in null else _vp(selectors), C.byref(err))
    return _seam_tables(h, err, [("selector_blocks", np.dtype((np.uint8, 8))), ("encoded_blocks", np.dtype((np.uint8, 8)))] + _WINDOWS)


def seam_pixel_tables(clusters, pixels, weights, total_pixels=None, null=()):
    err = C.c_char_p()
    total = pixels.shape[0] if total_pixels is None else total_pixels
    h = seam_translate_host().st_pixel_clusters(clusters.size, None if "clusters" in null else _vp(clusters), total, None if "pixels" in null else _vp(pixels),
                                                None if "weights" in null else _vp(weights), C.byref(err))
    return _seam_tables(h, err, [("texels", np.uint32), ("offsets", np.uint32), ("indices", np.uint32), ("reps", np.uint32), ("totals", np.uint64)])


def host_encode_uastc(blocks, flags):
    blocks = np.ascontiguousarray(blocks)
    n = blocks.shape[0]
    out = np.zeros((n, 16), np.uint8)
    uastc_host().hc_encode_uastc(ptr(blocks), n, flags, ptr(out))
    return out


def host_decode_uastc(packed, nbx=None, nby=None):
    """UASTC LDR 4x4 blocks (n, 16) -> texels: (n, 4, 4, 4) u8, or the (nby * 4, nbx * 4, 4) raster when the block grid is given. The host build of the
    product's own uastc_core.h (unpack + per-texel interpolation); pinned to the reference's unpack_uastc in tests/test_uastc_core_host.py."""
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1, 16)
    out = np.zeros((packed.shape[0], 4, 4, 4), np.uint8)
    assert uastc_host().hc_decode_uastc(ptr(packed), packed.shape[0], ptr(out)) == 1
    return out if nbx is None else blocks_to_raster(out, nbx, nby)


def blocks_to_raster(texels, nbx, nby):
    """(n, 4, 4, C) block-raster texels -> (nby * 4, nbx * 4, C)"""
    c = texels.shape[-1]
    return texels.reshape(nby, nbx, 4, 4, c).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, c)


def ref_transcode_uastc(blocks, target, high_quality=False, channels=(0, 3)):
    """The reference's per-block UASTC transcoder of `target` (a transcoder_texture_format value) over (n, 16) blocks, one call (harness version 3)
    -> ((n, bytes per block) uint8 with refused blocks zeroed, what the reference returned per block (n,) uint8)"""
    L = ref()
    assert hasattr(L, "ref_transcode_uastc"), "oracle/_ref/libref_harness.so is older than harness version 3"
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out, ok = np.zeros((n, {2: 8, 3: 16, 4: 8, 5: 16, 6: 16, 10: 16, 13: 64}[target]), np.uint8), np.zeros(n, np.uint8)
    refused = L.ref_transcode_uastc(ptr(blocks), n, target, int(high_quality), channels[0], channels[1], ptr(out), ptr(ok))
    assert refused == n - int(ok.sum())
    return out, ok


def ref_decode_uastc(packed):
    """the reference's unpack_uastc (transcoder/basisu_transcoder.cpp:15743) per block -> (n, 4, 4, 4) u8"""
    L = ref()
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1, 16)
    out = np.zeros((packed.shape[0], 4, 4, 4), np.uint8)
    for i in range(packed.shape[0]):
        assert L.ref_unpack_uastc(ptr(packed[i]), ptr(out[i])) == 1
    return out


def decode_etc1s_blocks(blocks, nbx, nby):
    """ETC1S blocks (n, 8) u8 in block-raster order -> (nby * 4, nbx * 4, 3) u8: differential mode with zero deltas, both sub-blocks share
    colour5 and the intensity table (etc_block::unpack_color5 / get_block_colors, etc.h:543-570), selector bit planes per etc.h:232-236."""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8)
    v = b.astype(np.uint64)
    word = np.zeros(b.shape[0], np.uint64)
    for i in range(8):
        word = (word << np.uint64(8)) | v[:, i]
    r5, g5, b5 = ((word >> np.uint64(s)) & np.uint64(31) for s in (59, 51, 43))
    inten = ((word >> np.uint64(37)) & np.uint64(7)).astype(np.int64)
    lo = (word & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    table = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80], [-106, -33, 33, 106],
                      [-183, -47, 47, 183]], np.int64)
    base = np.stack([(c.astype(np.int64) << 3) | (c.astype(np.int64) >> 2) for c in (r5, g5, b5)], axis=1)      # (n, 3)
    to_sel = np.array([2, 3, 1, 0], np.int64)
    out = np.zeros((b.shape[0], 4, 4, 3), np.uint8)
    for y in range(4):
        for x in range(4):
            bit = np.uint64(x * 4 + y)
            raw = ((lo >> bit) & np.uint64(1)) | (((lo >> (np.uint64(16) + bit)) & np.uint64(1)) << np.uint64(1))
            sel = to_sel[raw.astype(np.int64)]
            out[:, y, x, :] = np.clip(base + table[inten, sel][:, None], 0, 255).astype(np.uint8)
    return out.reshape(nby, nbx, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 3)


def decode_backend_blocks(encoder_blocks, endpoint_color5_inten, selector_blocks, nbx, nby):
    """What a transcoder to ETC1 decodes from the backend's output (the texture basis_compressor computes its m_basis_* stats on, comp.cpp:4194-4221):
    per block the endpoint / selector codebook entries the backend finally coded (its RDO may have replaced the frontend's choice). encoder_blocks:
    the (n, 4) u32 rows of Etc1sBackend.get("encoder_blocks") = (endpoint index, predictor, selector index, history index + 1), indices in the
    frontend's numbering; endpoint_color5_inten (k, 4) u8; selector_blocks (m, 8) u8 (selector bit planes in bytes 4-7)."""
    eb = np.ascontiguousarray(encoder_blocks).view(np.uint32).reshape(-1, 4)
    ep = np.ascontiguousarray(endpoint_color5_inten, np.uint8).reshape(-1, 4)[eb[:, 0]]
    sb = np.ascontiguousarray(selector_blocks, np.uint8).reshape(-1, 8)[eb[:, 2]]
    blk = np.zeros((eb.shape[0], 8), np.uint8)
    blk[:, 0:3] = ep[:, 0:3] << 3
    blk[:, 3] = (ep[:, 3] << 5) | (ep[:, 3] << 2) | 3    # both intensity tables, differential + flip bits (etc_block::is_etc1s)
    blk[:, 4:8] = sb[:, 4:8]
    return decode_etc1s_blocks(blk, nbx, nby)


def decode_backend_output(fe, be, nbx, nby):
    """decode_backend_blocks for an Etc1sFrontend + Etc1sBackend pair (one slice covering all blocks)"""
    prm = fe.get("endpoint_cluster_etc_params").reshape(-1, 16)[:, :4]
    return decode_backend_blocks(be.get("encoder_blocks"), prm, fe.get("optimized_cluster_selectors"), nbx, nby)


def psnr(a, b):
    """image_metrics::calc's PSNR over the given channels (enc.cpp:2155-2226): 20 log10(255 / rms), clamped to 100"""
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return 100.0 if mse == 0 else min(100.0, 20.0 * np.log10(255.0 / np.sqrt(mse)))


def save_png(path, img):
    """Minimal 8-bit RGBA PNG writer (test inputs for the reference CLI)."""
    import struct, zlib
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    pathlib.Path(path).write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def have_ref_cli():
    return (ORACLE_DIR / "_ref" / "basisu").exists()


def run_ref_cli(png_path, *args, ktx2=False):
    """The reference command line tool (oracle/_ref/basisu, built from /root/reference) on one PNG (or a list of PNGs: array layers, cubemap
    faces, video frames of ONE output file) -> the bytes of the .basis (or .ktx2) it writes."""
    import subprocess, tempfile, shutil
    paths = list(png_path) if isinstance(png_path, (list, tuple)) else [png_path]
    with tempfile.TemporaryDirectory() as d:
        names = []
        for i, p in enumerate(paths):
            names.append("in.png" if len(paths) == 1 else f"in{i}.png")
            shutil.copy(p, pathlib.Path(d) / names[-1])
        r = subprocess.run([str(ORACLE_DIR / "_ref" / "basisu"), "-ktx2" if ktx2 else "-basis", "-no_multithreading", *args, *names], cwd=d, capture_output=True, text=True, timeout=600)
        outs = sorted(pathlib.Path(d).glob("*.ktx2" if ktx2 else "*.basis"))
        assert r.returncode == 0 and len(outs) == 1, r.stdout[-2000:] + r.stderr[-2000:]
        return np.fromfile(outs[0], np.uint8)


def ktx2_file_key_values(data):
    """The key-value pairs of a KTX2 file (kvdByteOffset/Length of the header), without the alignment dummy key the writer adds itself."""
    import struct
    raw = np.asarray(data, np.uint8).tobytes()
    ofs, size = struct.unpack_from("<II", raw, 56)
    out, pos = [], ofs
    while pos < ofs + size:
        n = struct.unpack_from("<I", raw, pos)[0]
        body = raw[pos + 4:pos + 4 + n]
        k = body[:body.index(b"\0")]
        if not (k and set(k) == {127}):
            out.append((k.decode(), body[len(k) + 1:]))
        pos = ofs + (pos + 4 + n - ofs + 3) // 4 * 4
    return out


def basis_file_key_values(data):
    """The key-value pairs stored in a .basis file (basis_file_header::m_extended_file_ofs/size)."""
    import struct
    raw = np.asarray(data, np.uint8).tobytes()
    ofs, size = struct.unpack_from("<II", raw, 69)
    if not size:
        return []
    kv, out, pos = raw[ofs:ofs + size], [], 8
    for _ in range(struct.unpack_from("<I", kv, 2)[0]):
        kl, vl = kv[pos], struct.unpack_from("<I", kv, pos + 1)[0]
        out.append((kv[pos + 5:pos + 5 + kl].decode(), kv[pos + 5 + kl:pos + 5 + kl + vl]))
        pos += 5 + kl + vl
    return out


def block_metric_host():
    """csrc/host/block_metric.h (the backend's inner loops, one variant per instruction set) compiled for the host: tests/native/block_metric_host.cpp."""
    return native_libs.load("block_metric_host")


# g_uastc_huff_modes (transcoder/basisu_transcoder.cpp:14409-14413): the mode of a UASTC block from the low 7 bits of its first byte
UASTC_HUFF_MODES = [11, 0, 10, 3, 11, 15, 12, 7, 11, 18, 10, 5, 11, 14, 12, 9, 11, 0, 10, 4, 11, 16, 12, 8, 11, 18, 10, 6, 11, 2, 12, 13, 11, 0, 10, 3, 11, 17, 12, 7, 11, 18, 10, 5, 11, 14, 12,
                    9, 11, 0, 10, 4, 11, 1, 12, 8, 11, 18, 10, 6, 11, 2, 12, 13, 11, 0, 10, 3, 11, 19, 12, 7, 11, 18, 10, 5, 11, 14, 12, 9, 11, 0, 10, 4, 11, 16, 12, 8, 11, 18, 10, 6, 11, 2,
                    12, 13, 11, 0, 10, 3, 11, 17, 12, 7, 11, 18, 10, 5, 11, 14, 12, 9, 11, 0, 10, 4, 11, 1, 12, 8, 11, 18, 10, 6, 11, 2, 12, 13]
