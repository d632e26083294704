"""-m gpu: every image of a file transcoded by ONE launch -- bu_hip_k_transcode_uastc_slices / bu_hip_k_transcode_etc1s_slices (include/basisu_hip.h) and
transcode.transcode_file_images / transcode_etc1s_file_images on top of them. Expected bytes are the reference tool's (tests/golden/etc1s_transcode_vectors.npz,
uastc_transcode_vectors.npz, uastc_transcode_fuzz.npz) and, where the caller chooses the layout, the one-image entries' on the same arguments."""
import ctypes as C
import functools
import pathlib

import numpy as np
import pytest

import etc1s_transcode_helpers as E
import multi_image_helpers as M
import transcode_helpers as H
from basis_universal_amd import backend
from basis_universal_amd import transcode as T
from basis_universal_amd.transcode import NO_ALPHA_SLICE, TranscodeSlice

pytestmark = pytest.mark.gpu
HERE = pathlib.Path(__file__).resolve().parent
GUARD = 0xA5
ETC1S_TARGETS = [T.ETC1_RGB, T.BC1_RGB, T.RGBA32, T.RGB565, T.BGR565, T.RGBA4444]
UASTC_CASES = {"rgba32": (T.RGBA32, False), "astc": (T.ASTC_4x4_RGBA, False), "bc7": (T.BC7_RGBA, False), "bc1": (T.BC1_RGB, False), "bc1_hq": (T.BC1_RGB, True),
               "bc3": (T.BC3_RGBA, False), "bc3_hq": (T.BC3_RGBA, True), "bc4_r": (T.BC4_R, False), "bc5_ra": (T.BC5_RG, False)}
vp = C.c_void_p


@functools.lru_cache(maxsize=None)
def uastc_golden():
    return np.load(HERE / "golden" / "uastc_transcode_vectors.npz")


@functools.lru_cache(maxsize=None)
def uastc_fuzz():
    return np.load(HERE / "golden" / "uastc_transcode_fuzz.npz")


def records(specs):
    """[(first, alpha_first or None, out_offset, nbx, nby, w, h, pitch, rows)] -> the C array"""
    recs = (TranscodeSlice * len(specs))()
    for k, (first, alpha, off, nbx, nby, w, h, pitch, rows) in enumerate(specs):
        recs[k] = TranscodeSlice(first, NO_ALPHA_SLICE if alpha is None else alpha, off, nbx, nby, w, h, pitch, rows)
    return recs


def extent(ctx, spec, target, etc1s):
    return ctx.lib.transcode_slice_extent(C.byref(records([spec])[0]), target, int(etc1s))


class Uastc:
    """resident UASTC blocks and the two entries over them"""
    etc1s = False

    def __init__(self, ctx, blocks):
        self.ctx, self.n, self.d = ctx, blocks.shape[0], ctx.upload(np.ascontiguousarray(blocks, np.uint8))

    def close(self):
        self.ctx.free(self.d)

    def slices(self, recs, n, target, d_out, out_bytes, invalid, hq=False, ch=(-1, -1), n_inputs=None, d_in=None):
        return self.ctx.lib.k_transcode_uastc_slices(self.ctx.h, vp(self.d if d_in is None else d_in), self.n if n_inputs is None else n_inputs, recs, n, target, 32 if hq else 0,
                                                     ch[0], ch[1], vp(d_out), out_bytes, invalid)

    def one(self, spec, target, d_out, hq=False, ch=(-1, -1)):
        first, _alpha, _off, nbx, nby, w, h, pitch, rows = spec
        invalid = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.k_transcode_uastc(self.ctx.h, vp(self.d + 16 * first), nbx, nby, w, h, target, 32 if hq else 0, ch[0], ch[1], vp(d_out), pitch, rows,
                                                      C.byref(invalid)), "transcode_uastc")
        return invalid.value


class Etc1s:
    """resident palettes and whole index arrays, and the two entries over them"""
    etc1s = True

    def __init__(self, ctx, ep, sel_u32, ei, si):
        self.ctx, self.n_ep, self.n_sel, self.n = ctx, ep.shape[0], sel_u32.size, ei.size
        self.held = [ctx.upload(np.ascontiguousarray(a)) for a in (ep, sel_u32, ei.astype(np.uint16), si.astype(np.uint16))]

    def close(self):
        for p in self.held:
            self.ctx.free(p)

    def slices(self, recs, n, target, d_out, out_bytes, invalid, n_inputs=None, n_ep=None, **_):
        h = self.held
        return self.ctx.lib.k_transcode_etc1s_slices(self.ctx.h, vp(h[0]), self.n_ep if n_ep is None else n_ep, vp(h[1]), self.n_sel, vp(h[2]), vp(h[3]),
                                                     self.n if n_inputs is None else n_inputs, recs, n, target, vp(d_out), out_bytes, invalid)

    def one(self, spec, target, d_out, **_):
        first, alpha, _off, nbx, nby, w, h, pitch, rows = spec
        h_ = self.held
        a_ep, a_sel = (None, None) if alpha is None else (vp(h_[2] + 2 * alpha), vp(h_[3] + 2 * alpha))
        invalid = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.k_transcode_etc1s_counted(self.ctx.h, vp(h_[0]), self.n_ep, vp(h_[1]), self.n_sel, vp(h_[2] + 2 * first), vp(h_[3] + 2 * first), a_ep, a_sel,
                                                              nbx, nby, w, h, target, vp(d_out), pitch, rows, C.byref(invalid)), "transcode_etc1s_counted")
        return invalid.value


def run(ctx, codec, specs, target, total, want_counts=True, **kw):
    """one whole-file call into a guard-filled buffer of `total` bytes -> (return value, the buffer afterwards, per-slice counts or None)"""
    d_out = ctx.upload(np.full(total, GUARD, np.uint8))
    try:
        invalid = (C.c_uint32 * len(specs))(*([0xFFFFFFFF] * len(specs))) if want_counts else None
        ok = codec.slices(records(specs), len(specs), target, d_out, total, invalid, **kw)
        return ok, ctx.download(d_out, (total,), np.uint8), (list(invalid) if want_counts else None)
    finally:
        ctx.free(d_out)


def packed(ctx, shapes, target, etc1s, firsts, alphas=None):
    """tight records for (nbx, nby, w, h) shapes, outputs packed in order at 16-byte steps -> (specs, total bytes)"""
    specs, at = [], 0
    for k, (nbx, nby, w, h) in enumerate(shapes):
        spec = (int(firsts[k]), None if alphas is None else alphas[k], at, nbx, nby, w, h, 0, 0)
        specs.append(spec)
        at += (extent(ctx, spec, target, etc1s) + 15) & ~15
    return specs, at


def synthetic_state(n_blocks, seed, n_ep=40, n_sel=50):
    rng = np.random.default_rng(seed)
    ep = np.stack([rng.integers(0, 32, n_ep), rng.integers(0, 32, n_ep), rng.integers(0, 32, n_ep), rng.integers(0, 8, n_ep)], 1).astype(np.uint8)
    sel = E.selector_palette_u32(rng.integers(0, 4, (n_sel, 16)).astype(np.uint8))
    return ep, sel, rng.integers(0, n_ep, n_blocks).astype(np.uint16), rng.integers(0, n_sel, n_blocks).astype(np.uint16)


# ---------------------------------------------------------------- 1. ETC1S files against the reference tool

def _etc1s_files():
    _, meta = E.golden()
    return [f["name"] for f in meta["files"]]


@pytest.mark.parametrize("name", _etc1s_files())
def test_etc1s_golden_files_every_target(hip_ctx, name):
    arrays, _ = E.golden()
    data = arrays["file_" + name]
    images = T.read_etc1s_file(data)["images"]
    for target in ETC1S_TARGETS:
        got = T.transcode_etc1s_file_images(hip_ctx, data, target)
        assert len(got) == len(images)
        for im, out in zip(images, got):
            key = E.image_key(name, im["level"], im["layer"], im["face"])
            if target in T.ETC1S_BYTES_PER_BLOCK:
                exp = arrays[key + ("_etc1" if target == T.ETC1_RGB else "_bc1")]
            else:
                rgba = E.expected_rgba(arrays, key, im["width"], im["height"], im["num_blocks_x"], im["num_blocks_y"])
                exp = rgba if target == T.RGBA32 else E.pack_pixels(rgba, target)
            assert out.shape == exp.shape and out.dtype == exp.dtype and (out == exp).all(), (key, target)


# ---------------------------------------------------------------- 2. UASTC block sets cut where waves and workgroups end

CUTS = [1, 1, 1, 63, 1, 64, 65, 1, 255, 257, 1]


def _cut_shapes():
    """one block row per count, then the even counts again as 2-row grids"""
    return [(c, 1, 4 * c, 4) for c in CUTS] + [(c // 2, 2, 2 * c, 8) for c in CUTS if c % 2 == 0]


@pytest.mark.parametrize("which", ["level3", "level2", "default_l2"])
def test_uastc_block_sets_cut_at_wave_and_workgroup_boundaries(hip_ctx, which):
    g = uastc_golden()
    shapes = _cut_shapes()
    counts = [s[0] * s[1] for s in shapes]
    firsts = np.concatenate([[0], np.cumsum(counts)])
    assert firsts[-1] <= g[f"{which}_blocks"].shape[0]
    codec = Uastc(hip_ctx, g[f"{which}_blocks"])
    try:
        for name, (target, hq) in UASTC_CASES.items():
            specs, total = packed(hip_ctx, shapes, target, False, firsts)
            ok, raw, invalid = run(hip_ctx, codec, specs, target, total, hq=hq)
            assert ok == 1 and invalid == [0] * len(shapes), (name, hip_ctx.lib.last_error(hip_ctx.h))
            exp_all = g[f"{which}_{name}"]
            for k, (spec, (nbx, nby, w, h)) in enumerate(zip(specs, shapes)):
                exp = exp_all[firsts[k]:firsts[k + 1]]
                if target == T.RGBA32:
                    exp = H.to_raster(exp.reshape(-1, 4, 4, 4), nbx, nby, w, h)
                got = raw[spec[2]:spec[2] + exp.size].reshape(exp.shape)
                assert (got == exp).all(), (name, k)
    finally:
        codec.close()


# ---------------------------------------------------------------- 3. whole files against the one-image path

def _multi_files(uastc):
    g, _ = M.load()
    names = sorted(k[len("file_"):] for k in g.files if k.startswith("file_") and ("_uastc_" in k) == uastc)
    return [n for n in names if "video" not in n or uastc]   # reading ETC1S video back is not supported


@pytest.mark.parametrize("name", _multi_files(True))
def test_uastc_files_equal_the_one_image_path(hip_ctx, name):
    g, _ = M.load()
    data = g["file_" + name]
    images = T.read_uastc_file(data.tobytes())["images"]
    assert len(images) > 1
    for target, hq in ((T.RGBA32, False), (T.BC3_RGBA, True)):
        got = T.transcode_file_images(hip_ctx, data, target, high_quality=hq)
        assert len(got) == len(images)
        for im, out in zip(images, got):
            exp = T.transcode_file(hip_ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"], high_quality=hq)
            assert out.shape == exp.shape and (out == exp).all(), (name, target, im["level"], im["layer"], im["face"])
    # the caller's buffer: the layout comes back and the bytes are there
    layout, total = T.image_layout(images, T.BC7_RGBA, etc1s=False)
    d_out = hip_ctx.upload(np.full(total, GUARD, np.uint8))
    try:
        assert T.transcode_file_images(hip_ctx, data, T.BC7_RGBA, out_device=d_out) == (layout, total)
        raw = hip_ctx.download(d_out, (total,), np.uint8)
    finally:
        hip_ctx.free(d_out)
    for im, e in zip(images, layout):
        exp = T.transcode_file(hip_ctx, data, T.BC7_RGBA, level=im["level"], layer=im["layer"], face=im["face"])
        assert (raw[e["offset"]:e["offset"] + e["nbytes"]].reshape(e["shape"]) == exp).all()


@pytest.mark.parametrize("name", _multi_files(False))
def test_etc1s_files_equal_the_one_image_path(hip_ctx, name):
    g, _ = M.load()
    data = g["file_" + name]
    images = T.read_etc1s_file(data)["images"]
    assert len(images) > 1
    for target in (T.RGBA32, T.BC1_RGB):
        got = T.transcode_etc1s_file_images(hip_ctx, data, target)
        assert len(got) == len(images)
        for im, out in zip(images, got):
            exp = T.transcode_etc1s_file(hip_ctx, data, target, level=im["level"], layer=im["layer"], face=im["face"])
            assert out.shape == exp.shape and (out == exp).all(), (name, target, im["level"], im["layer"], im["face"])
    layout, total = T.image_layout(images, T.RGBA4444, etc1s=True)
    d_out = hip_ctx.upload(np.full(total, GUARD, np.uint8))
    try:
        assert T.transcode_etc1s_file_images(hip_ctx, data, T.RGBA4444, out_device=d_out) == (layout, total)
        raw = hip_ctx.download(d_out, (total,), np.uint8)
    finally:
        hip_ctx.free(d_out)
    for im, e in zip(images, layout):
        exp = T.transcode_etc1s_file(hip_ctx, data, T.RGBA4444, level=im["level"], layer=im["layer"], face=im["face"])
        assert (raw[e["offset"]:e["offset"] + e["nbytes"]].view(np.uint16).reshape(e["shape"]) == exp).all()


# ---------------------------------------------------------------- 4. a layout the caller chooses

GRIDS = [(5, 3), (1, 1), (17, 16), (2, 7), (3, 5)]   # 272 blocks in the third: more than a workgroup; the last reads the first's range again


def _chosen_layout(ctx, target, etc1s, pixels, with_alpha):
    """ragged sizes, a padded pitch and cut rows on slice 2 (pixel targets), 48-byte gaps, inputs in descending order, slice 4 on slice 0's blocks"""
    counts = [nbx * nby for nbx, nby in GRIDS]
    firsts, at = [], 0
    for c in reversed(counts[:4]):
        firsts.insert(0, at)
        at += c
    firsts.append(firsts[0])
    assert firsts[:4] == sorted(firsts[:4], reverse=True)
    alphas = [at if with_alpha else None, None, at + 3 if with_alpha else None, None, None]
    n_inputs = at + 3 + counts[2]
    specs, off = [], 32
    for k, (nbx, nby) in enumerate(GRIDS):
        w, h = 4 * nbx - 3, 4 * nby - 1
        pitch, rows = (w + 5, h - 2) if pixels and k == 2 else (0, 0)
        spec = (firsts[k], alphas[k], off, nbx, nby, w, h, pitch, rows)
        specs.append(spec)
        off += ((extent(ctx, spec, target, etc1s) + 15) & ~15) + 48
    return specs, off, n_inputs


def _expected_from_one_image_calls(ctx, codec, specs, target, total, **kw):
    exp = np.full(total, GUARD, np.uint8)
    for spec in specs:
        n = extent(ctx, spec, target, codec.etc1s)
        d_tmp = ctx.upload(np.full(n, GUARD, np.uint8))
        try:
            assert codec.one(spec, target, d_tmp, **kw) == 0
            exp[spec[2]:spec[2] + n] = ctx.download(d_tmp, (n,), np.uint8)
        finally:
            ctx.free(d_tmp)
    return exp


@pytest.mark.parametrize("name", ["rgba32", "bc1_hq", "bc7", "bc5_ra"])
def test_uastc_layout_the_caller_chooses(hip_ctx, name):
    target, hq = UASTC_CASES[name]
    specs, total, n_inputs = _chosen_layout(hip_ctx, target, False, target == T.RGBA32, False)
    ch = (1, 2) if target == T.BC5_RG else (-1, -1)
    codec = Uastc(hip_ctx, uastc_golden()["level3_blocks"][:n_inputs])
    try:
        exp = _expected_from_one_image_calls(hip_ctx, codec, specs, target, total, hq=hq, ch=ch)
        assert (exp[:32] == GUARD).all() and (exp != GUARD).sum() > total // 4
        ok, raw, invalid = run(hip_ctx, codec, specs, target, total, hq=hq, ch=ch)
        assert ok == 1 and invalid == [0] * len(specs), hip_ctx.lib.last_error(hip_ctx.h)
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (bad[:8], total)
    finally:
        codec.close()


@pytest.mark.parametrize("target", ETC1S_TARGETS)
def test_etc1s_layout_the_caller_chooses(hip_ctx, target):
    pixels = target in T.ETC1S_BYTES_PER_PIXEL
    specs, total, n_inputs = _chosen_layout(hip_ctx, target, True, pixels, True)
    codec = Etc1s(hip_ctx, *synthetic_state(n_inputs, 31))
    try:
        exp = _expected_from_one_image_calls(hip_ctx, codec, specs, target, total)
        assert (exp[:32] == GUARD).all() and (exp != GUARD).sum() > total // 4
        ok, raw, invalid = run(hip_ctx, codec, specs, target, total)
        assert ok == 1 and invalid == [0] * len(specs), hip_ctx.lib.last_error(hip_ctx.h)
        bad = np.flatnonzero(raw != exp)
        assert bad.size == 0, (bad[:8], total)
    finally:
        codec.close()


# ---------------------------------------------------------------- 5. per-slice invalid counts

FIVE = [(9, 2, 36, 8), (70, 1, 280, 4), (1, 1, 4, 4), (20, 15, 80, 60), (3, 3, 10, 11)]   # slice 3: 300 blocks, over a workgroup's end


def _planted(counts, seed):
    """block indices (in table order) to spoil: a few in slice 1, more in slice 3 -> (indices, [0, k1, 0, k3, 0])"""
    firsts = np.concatenate([[0], np.cumsum(counts)])
    rng = np.random.default_rng(seed)
    in1 = firsts[1] + rng.choice(counts[1], 5, replace=False)
    in3 = firsts[3] + np.concatenate([[0, counts[3] - 1], 1 + rng.choice(counts[3] - 2, 9, replace=False)])
    return firsts, np.sort(np.concatenate([in1, in3])), [0, 5, 0, 11, 0]


def _check_planted(ctx, codec, specs, target, total, clean, bad_blocks, firsts, want_counts, unit, **kw):
    ok, raw, invalid = run(ctx, codec, specs, target, total, **kw)
    assert ok == 1 and invalid == want_counts, (invalid, ctx.lib.last_error(ctx.h))
    ok2, raw2, none = run(ctx, codec, specs, target, total, want_counts=False, **kw)   # NULL: the call returns 1 and writes the same
    assert ok2 == 1 and none is None and (raw2 == raw).all()
    for k, spec in enumerate(specs):
        nbx, nby, w, h = spec[3:7]
        mine = bad_blocks[(bad_blocks >= firsts[k]) & (bad_blocks < firsts[k + 1])] - firsts[k]
        n = extent(ctx, spec, target, codec.etc1s)
        got, exp = raw[spec[2]:spec[2] + n], clean[spec[2]:spec[2] + n].copy()
        if unit:   # block target: `unit` bytes per block
            exp.reshape(-1, unit)[mine] = 0
        else:      # pixel target: the tile's pixels inside the image
            px = n // (w * h)
            view = exp.reshape(h, w, px)
            for b in mine:
                view[4 * (b // nbx):4 * (b // nbx) + 4, 4 * (b % nbx):4 * (b % nbx) + 4] = 0
        assert (got == exp).all(), (k, target)
    return raw


@pytest.mark.parametrize("target", [T.BC1_RGB, T.RGBA32, T.RGB565])
def test_etc1s_invalid_blocks_are_counted_per_slice(hip_ctx, target):
    counts = [s[0] * s[1] for s in FIVE]
    firsts, bad, want = _planted(counts, 3)
    ep, sel, ei, si = synthetic_state(int(firsts[-1]), 17)
    bad_ei, bad_si = ei.copy(), si.copy()
    bad_ei[bad[::2]] = ep.shape[0]      # the first index past the endpoint palette
    bad_si[bad[1::2]] = 65535           # far past the selector palette
    specs, total = packed(hip_ctx, FIVE, target, True, firsts)
    good, spoiled = Etc1s(hip_ctx, ep, sel, ei, si), Etc1s(hip_ctx, ep, sel, bad_ei, bad_si)
    try:
        ok, clean, invalid = run(hip_ctx, good, specs, target, total)
        assert ok == 1 and invalid == [0] * 5
        _check_planted(hip_ctx, spoiled, specs, target, total, clean, bad, firsts, want, 8 if target == T.BC1_RGB else 0)
    finally:
        good.close()
        spoiled.close()


@pytest.mark.parametrize("name", ["bc1", "rgba32", "astc"])
def test_uastc_invalid_blocks_are_counted_per_slice(hip_ctx, name):
    target, hq = UASTC_CASES[name]
    counts = [s[0] * s[1] for s in FIVE]
    firsts, bad, want = _planted(counts, 4)
    f = uastc_fuzz()
    blocks = uastc_golden()["level3_blocks"][:firsts[-1]].copy()
    invalid_blocks = f["blocks"][f["valid"] == 0]
    assert invalid_blocks.shape[0] >= bad.size
    spoiled_blocks = blocks.copy()
    spoiled_blocks[bad] = invalid_blocks[:: invalid_blocks.shape[0] // bad.size][:bad.size]
    specs, total = packed(hip_ctx, FIVE, target, False, firsts)
    good, spoiled = Uastc(hip_ctx, blocks), Uastc(hip_ctx, spoiled_blocks)
    try:
        ok, clean, invalid = run(hip_ctx, good, specs, target, total, hq=hq)
        assert ok == 1 and invalid == [0] * 5
        _check_planted(hip_ctx, spoiled, specs, target, total, clean, bad, firsts, want, 0 if target == T.RGBA32 else T.BYTES_PER_BLOCK[target], hq=hq)
    finally:
        good.close()
        spoiled.close()


def test_python_calls_raise_naming_the_lowest_slice(hip_ctx, monkeypatch):
    counts = [s[0] * s[1] for s in FIVE]
    firsts, bad, want = _planted(counts, 5)
    f = uastc_fuzz()
    blocks = uastc_golden()["level3_blocks"][:firsts[-1]].copy()
    invalid_blocks = f["blocks"][f["valid"] == 0]
    blocks[bad] = invalid_blocks[:bad.size]
    data = backend.uastc_basis_file(blocks, [(int(firsts[k]), nbx, nby, w, h, k, 0, 0) for k, (nbx, nby, w, h) in enumerate(FIVE)])   # five images of a .basis file
    with pytest.raises(T.InvalidBlocksError, match="slice 1") as e:
        T.transcode_file_images(hip_ctx, data, T.BC7_RGBA)
    assert (e.value.count, e.value.slice, e.value.per_slice) == (16, 1, want)
    # ETC1S: the host decoder refuses a file with an index past its palette, so the indices are spoiled behind it
    arrays, _ = E.golden()
    mip = arrays["file_mip_basis"]
    decode = T._decode_etc1s

    def spoiled(data, header_only, whole=False):
        d = decode(data, header_only, whole)
        if whole:
            ims = d["images"]
            d["_endpoint_indices"] = d["_endpoint_indices"].copy()
            d["_endpoint_indices"][[ims[1]["_first"] + 2, ims[1]["_first"] + 7, ims[3]["_first"]]] = 65535
        return d
    monkeypatch.setattr(T, "_decode_etc1s", spoiled)
    with pytest.raises(T.InvalidBlocksError, match="slice 1") as e:
        T.transcode_etc1s_file_images(hip_ctx, mip, T.RGBA32)
    assert (e.value.count, e.value.slice, e.value.per_slice) == (3, 1, [0, 2, 0, 1, 0])


# ---------------------------------------------------------------- 6. refusals

def _refusals(etc1s, pixel_target, block_target):
    """(what is wrong, target, the records, keyword arguments of the call, words of the reason) on a 4-slice table of 2 x 2 blocks; inputs: 64"""
    size = 256 if not etc1s else 64 * (4 if pixel_target == T.RGBA32 else 2)
    def table(**change):
        specs = [[4 * k, None, 512 * k, 2, 2, 0, 0, 0, 0] for k in range(4)]
        for k, fields in change.items():
            for i, v in fields.items():
                specs[int(k[1:])][i] = v
        return [tuple(s) for s in specs]
    FIRST, ALPHA, OFF, NBX, NBY, W, H, PITCH, ROWS = range(9)
    cases = [("no slices", pixel_target, [], {}, "no slices"),
             ("zero blocks across", pixel_target, table(s1={NBX: 0}), {}, "slice 1: zero blocks"),
             ("zero blocks down", block_target, table(s3={NBY: 0}), {}, "slice 3: zero blocks"),
             ("too many blocks across", block_target, table(s0={NBX: 16385}), {}, "slice 0: 16385 x 2 blocks is too many"),
             ("too many blocks down", pixel_target, table(s2={NBY: 16385}), {}, "slice 2: 2 x 16385 blocks is too many"),
             ("pixels wider than the blocks", pixel_target, table(s1={W: 9}), {}, "slice 1: 9 x 8 pixels do not fit 2 x 2 blocks"),
             ("pixels taller than the blocks", block_target, table(s1={H: 9}), {}, "slice 1: 8 x 9 pixels do not fit 2 x 2 blocks"),
             ("pitch below the width", pixel_target, table(s2={W: 7, PITCH: 6}), {}, "slice 2: row pitch 6 is less than the width 7"),
             ("pitch for a block target", block_target, table(s1={PITCH: 8}), {}, "slice 1: row pitch 8 / rows 0 given for a block target"),
             ("rows for a block target", block_target, table(s1={ROWS: 8}), {}, "slice 1: row pitch 0 / rows 8 given for a block target"),
             ("input range past the end", pixel_target, table(s3={FIRST: 61}), {}, "slice 3: " + ("indices" if etc1s else "blocks") + " 61..65 are past the 64 given"),
             ("fewer inputs than the table reads", block_target, table(), {"n_inputs": 15}, "slice 3: " + ("indices" if etc1s else "blocks") + " 12..16 are past the 15 given"),
             ("first_block past everything", block_target, table(s0={FIRST: 2 ** 63}), {}, "slice 0"),
             ("out_offset not aligned", pixel_target, table(s1={OFF: 520}), {}, "slice 1: out_offset 520 is not 16-byte aligned"),
             ("output past out_bytes", pixel_target, table(s3={OFF: 2048 - size + 16}), {}, "slice 3: its output, bytes"),
             ("out_offset past out_bytes", block_target, table(s3={OFF: 4096}), {}, "slice 3: its output, bytes 4096..4128, ends past out_bytes = 2048"),
             ("outputs overlap", pixel_target, table(s2={OFF: 512 + size - 16}), {}, "slice 2: out_offset"),
             ("outputs descend", block_target, table(s1={OFF: 1024}, s2={OFF: 512}), {}, "slice 2: out_offset 512 lies before the end of slice 1's output (1056)")]
    if etc1s:
        cases += [("alpha range past the end", T.RGBA32, table(s1={ALPHA: 62}), {}, "slice 1: alpha indices 62..66 are past the 64 given"),
                  ("no endpoints", pixel_target, table(), {"n_ep": 0}, "palettes of 0 endpoints"),
                  ("too many endpoints", pixel_target, table(), {"n_ep": 65536}, "palettes of 65536 endpoints")]
    else:
        cases += [("an alpha slice for UASTC", pixel_target, table(s2={ALPHA: 0}), {}, "slice 2: alpha_first_block is set"),
                  ("channel out of range", T.BC5_RG, table(), {"ch": (1, 4)}, "channel out of range")]
    return cases


def _refused(ctx, codec, specs, target, words, **kw):
    ok, raw, _ = run(ctx, codec, specs, target, 2048, **kw)
    err = ctx.lib.last_error(ctx.h)
    assert ok == 0 and words in err and (raw == GUARD).all(), (words, ok, err)


GOOD = [(4 * k, None, 512 * k, 2, 2, 0, 0, 0, 0) for k in range(4)]


@pytest.mark.parametrize("etc1s", [False, True])
def test_argument_errors_are_refused_by_name_and_write_nothing(hip_ctx, etc1s):
    codec = Etc1s(hip_ctx, *synthetic_state(64, 9)) if etc1s else Uastc(hip_ctx, uastc_golden()["level3_blocks"][:64])
    fn = "transcode_etc1s_slices" if etc1s else "transcode_uastc_slices"
    try:
        for what, target, specs, kw, words in _refusals(etc1s, T.RGBA32, T.BC1_RGB):
            _refused(hip_ctx, codec, specs, target, fn + ": " + words, **kw)
        # null pointers, a misaligned output, more than 2^30 blocks in all
        d_out = hip_ctx.upload(np.full(2048, GUARD, np.uint8))
        try:
            recs, invalid = records(GOOD), (C.c_uint32 * 4)()
            assert codec.slices(None, 4, T.RGBA32, d_out, 2048, invalid) == 0 and "null pointer" in hip_ctx.lib.last_error(hip_ctx.h)
            assert codec.slices(recs, 4, T.RGBA32, None, 2048, invalid) == 0 and "null pointer" in hip_ctx.lib.last_error(hip_ctx.h)
            assert codec.slices(recs, 4, T.RGBA32, d_out + 8, 2040, invalid) == 0 and "the output is not 16-byte aligned" in hip_ctx.lib.last_error(hip_ctx.h)
            if not etc1s:
                assert codec.slices(recs, 4, T.RGBA32, d_out, 2048, invalid, d_in=0) == 0 and "null pointer" in hip_ctx.lib.last_error(hip_ctx.h)
                assert codec.slices(recs, 4, T.RGBA32, d_out, 2048, invalid, d_in=codec.d + 8) == 0 and "the blocks are not 16-byte aligned" in hip_ctx.lib.last_error(hip_ctx.h)
            big = records([(0, None, k * 2 ** 31, 16384, 16384, 0, 0, 0, 0) for k in range(5)])   # 5 x 2^28 blocks, all reading the same range: refused on the count alone
            assert codec.slices(big, 5, T.BC1_RGB, d_out, 2 ** 40, None, n_inputs=2 ** 28) == 0 and "more than 2^30 blocks" in hip_ctx.lib.last_error(hip_ctx.h)
            assert (hip_ctx.download(d_out, (2048,), np.uint8) == GUARD).all()
            # and the table as it stands is accepted
            assert codec.slices(recs, 4, T.BC1_RGB, d_out, 2048, invalid) == 1 and list(invalid) == [0, 0, 0, 0]
        finally:
            hip_ctx.free(d_out)
    finally:
        codec.close()


def test_targets_a_codec_refuses_are_refused_with_the_existing_text(hip_ctx):
    codec = Uastc(hip_ctx, uastc_golden()["level3_blocks"][:64])
    try:
        for target in (0, 1, 8, 14, 16, 22):
            _refused(hip_ctx, codec, GOOD, target, f"transcode_uastc: target {target} is not supported (RGBA32, ASTC 4x4, BC1, BC3, BC4, BC5, BC7 are)")
            assert hip_ctx.lib.transcode_slice_extent(C.byref(records(GOOD)[0]), target, 0) == 0
            with pytest.raises(ValueError, match=rf"transcode target {target} is not supported \(supported: \[2, 3, 4, 5, 6, 10, 13\]\)"):
                T.transcode_file_images(M.Untouchable(), M.load()[0]["file_c_uastc_cubemap_alpha_ktx2"], target)
    finally:
        codec.close()
    codec = Etc1s(hip_ctx, *synthetic_state(64, 9))
    arrays, _ = E.golden()
    try:
        for target, name in ((1, "ETC2_RGBA"), (3, "BC3_RGBA"), (4, "BC4_R"), (5, "BC5_RG"), (6, "BC7_RGBA"), (8, "PVRTC1_4_RGB"), (10, "ASTC_4x4_RGBA"), (11, "ATC_RGB"), (17, "FXT1_RGB"),
                             (20, "ETC2_EAC_R11"), (99, "unknown")):
            _refused(hip_ctx, codec, GOOD, target, f"transcode_etc1s: target {target} ({name}) is not supported (supported: ETC1_RGB (0), BC1_RGB (2), RGBA32 (13), RGB565 (14), "
                                                   "BGR565 (15), RGBA4444 (16))")
            assert hip_ctx.lib.transcode_slice_extent(C.byref(records(GOOD)[0]), target, 1) == 0
            with pytest.raises(ValueError, match=rf"ETC1S transcode target {target} \({name}\) is not supported"):
                T.transcode_etc1s_file_images(M.Untouchable(), arrays["file_mip_basis"], target)
    finally:
        codec.close()
