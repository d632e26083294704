"""What the source-preparation tests and their golden generator (tools/gen_golden_source_prep.py) share: the seeded inputs, the case list with the reference tool's
flags, THE table that maps those flags to keyword arguments of compress(), the 2^24-colour image and its band digests, and the g++ build of csrc/source_prep.h
(tests/native/source_prep_host.cpp). The expected values are what the tool wrote: there is no tolerance anywhere, every comparison is equality of bytes."""
import functools
import hashlib
import json
import pathlib

import numpy as np

import helpers
import native_libs

ROOT = pathlib.Path(__file__).resolve().parent.parent
NATIVE = native_libs.NATIVE
native_libs.CHECKERS.setdefault("source_prep_host", (NATIVE / "libsource_prep_host.so", NATIVE / "source_prep_host.cpp", "HOST_API", "g++"))

GOLDEN = ROOT / "tests" / "golden" / "source_prep_vectors.npz"
DIGESTS = ROOT / "tests" / "golden" / "source_prep_digests.json"
ALL_SIDE, BAND_ROWS = 4096, 64          # the 2^24-colour image and the rows per digest


# ---------------------------------------------------------------- inputs

def _synth(w, h, seed):
    return np.ascontiguousarray(helpers.synth((w + 3) // 4 * 4, (h + 3) // 4 * 4, seed)[:h, :w])   # synth takes multiples of 4


def normal_map_image(w, h, seed):
    """A tangent-space normal map, opaque: unit normals of a bumpy surface, of which about a fifth are scaled off unit length (both ways, beyond the .077 band), a tenth
    are exactly (128, 128, 128) and a tenth lie within .077 of zero -> ((h, w, 4) u8, {"off_unit", "grey", "near_zero"} pixel counts)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    n = np.stack([0.6 * np.sin(x / 2.3 + seed), 0.6 * np.cos(y / 1.7), np.ones_like(x)], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    kind = rng.permutation(w * h).reshape(h, w) % 10      # 0, 1: off unit length; 2: grey; 3: near zero; the rest: unit
    scale = np.where(kind == 0, 0.55, np.where(kind == 1, 1.0, 1.0))
    n = n * scale[..., None]
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., :3] = np.clip(np.floor((n + 1.0) * 127.5 + 0.5), 0, 255).astype(np.uint8)
    img[kind == 1, :3] = np.clip(img[kind == 1, :3].astype(np.int64) + np.array([40, 40, 0]), 0, 255).astype(np.uint8)   # longer than 1 before the clamp
    img[kind == 2, :3] = 128
    img[kind == 3, :3] = 128 + rng.integers(-4, 5, (int((kind == 3).sum()), 3))
    return np.ascontiguousarray(img), {"off_unit": int((kind <= 1).sum()), "grey": int((kind == 2).sum()), "near_zero": int((kind == 3).sum())}


def alpha_image(w, h, seed):
    """helpers.synth with an alpha that is neither constant nor a copy of a colour channel; some of it is 255"""
    img = _synth(w, h, seed)
    y, x = np.mgrid[0:h, 0:w]
    img[..., 3] = np.clip(40 + x * 11 + y * 17, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img)


def opaque_image(w, h, seed):
    return _synth(w, h, seed)


SOURCES = {"normal": lambda w, h, seed: normal_map_image(w, h, seed)[0], "alpha": alpha_image, "opaque": opaque_image}


def source_image(case):
    img = SOURCES[case["source"]](case["w"], case["h"], case["seed"])
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------- the cases: the tool's flags, as the generator passes them

def _single_options():
    """(name, source, (w, h), flags): each option on its own"""
    return [("renorm", "normal", (21, 13), ["-renorm"]),
            ("swizzle_bgra", "alpha", (21, 13), ["-swizzle", "bgra"]),
            ("swizzle_1032", "alpha", (4, 1), ["-swizzle", "1032"]),
            ("separate_rg", "normal", (21, 13), ["-separate_rg_to_color_alpha"]),
            ("force_alpha", "opaque", (21, 13), ["-force_alpha"]),
            ("no_alpha", "alpha", (21, 13), ["-no_alpha"]),
            ("y_flip", "alpha", (21, 13), ["-y_flip"]),
            ("y_flip_4x1", "alpha", (4, 1), ["-y_flip"]),
            ("resample", "alpha", (21, 13), ["-resample", "12", "9"]),
            ("resample_factor", "opaque", (20, 28), ["-resample_factor", "0.6"]),
            ("mip_filter", "alpha", (20, 28), ["-mipmap", "-mip_filter", "box"]),
            ("mip_scale", "opaque", (20, 28), ["-mipmap", "-mip_scale", "1.25"]),
            ("mip_clamp", "opaque", (20, 28), ["-mipmap", "-mip_clamp"]),
            ("mip_linear", "alpha", (20, 28), ["-mipmap", "-mip_linear"]),
            ("mip_renorm", "normal", (20, 28), ["-mipmap", "-mip_renorm"]),
            ("mip_slow", "opaque", (21, 13), ["-mipmap", "-mip_slow"]),
            ("mip_smallest", "opaque", (20, 28), ["-mipmap", "-mip_smallest", "4"]),
            ("normal_map", "normal", (21, 13), ["-normal_map"])]


def case_list():
    """[{"name", "source", "w", "h", "seed", "uastc", "ext", "flags"}]: every single option with both codecs (ETC1S .basis, UASTC .ktx2), then the combinations"""
    out, seed = [], 9100

    def add(name, source, size, uastc, ext, flags):
        nonlocal seed
        out.append({"name": name, "source": source, "w": size[0], "h": size[1], "seed": seed, "uastc": uastc, "ext": ext, "flags": list(flags)})
        seed += 1
    for name, source, size, flags in _single_options():
        add("etc1s_" + name, source, size, False, "basis", flags)
        add("uastc_" + name, source, size, True, "ktx2", flags)
    add("etc1s_no_rdo", "opaque", (20, 28), False, "basis", ["-no_selector_rdo", "-no_endpoint_rdo"])
    add("etc1s_no_selector_rdo", "opaque", (20, 28), False, "ktx2", ["-no_selector_rdo"])
    add("etc1s_no_endpoint_rdo", "opaque", (20, 28), False, "basis", ["-no_endpoint_rdo"])
    add("combo_renorm_flip_rrrg", "normal", (21, 13), True, "ktx2", ["-renorm", "-y_flip", "-swizzle", "rrrg"])
    add("combo_normal_map_mips", "normal", (20, 28), False, "basis", ["-normal_map", "-mipmap", "-mip_renorm", "-mip_filter", "box", "-mip_clamp"])
    add("combo_mips", "alpha", (20, 28), False, "ktx2", ["-mipmap", "-mip_filter", "lanczos4", "-mip_scale", "1.25", "-mip_slow", "-mip_smallest", "4", "-mip_linear"])
    add("combo_resample_uastc", "alpha", (21, 13), True, "basis", ["-resample", "12", "9"])
    add("combo_resample_factor_etc1s", "alpha", (21, 13), False, "ktx2", ["-resample_factor", "0.6"])
    add("combo_no_alpha_uastc_basis", "alpha", (20, 28), True, "basis", ["-no_alpha"])
    add("combo_force_alpha_uastc_basis", "opaque", (20, 28), True, "basis", ["-force_alpha", "-y_flip"])
    add("combo_force_and_no_alpha", "alpha", (21, 13), False, "basis", ["-no_alpha", "-force_alpha"])
    # -resample where it does not shrink both axes: above the source size, one axis up and one down, the source's own size (image_resample's shortcut: a copy), a
    # factor above 1 -- the resampler's y-first pass order and its magnification lists. After everything above, so that the seeds of the older cases stay.
    for name, flags in _RESAMPLE_UPWARDS:
        for uastc, source in ((False, "alpha"), (True, "opaque")):
            for ext in ("basis", "ktx2"):
                add(f"{'uastc' if uastc else 'etc1s'}_{name}_{ext}", source, (21, 13), uastc, ext, flags)
    return out


_RESAMPLE_UPWARDS = [("resample_up", ["-resample", "40", "30"]), ("resample_mixed", ["-resample", "30", "9"]), ("resample_same", ["-resample", "21", "13"]),
                     ("resample_factor_up", ["-resample_factor", "1.7"])]


# flag -> (how many values follow it, what it sets). THE table: the generator passes the flags to the tool, the tests pass what this gives to compress().
_FLAGS = {
    "-renorm": (0, lambda: {"renormalize": True}),
    "-swizzle": (1, lambda s: {"swizzle": s}),
    "-separate_rg_to_color_alpha": (0, lambda: {"swizzle": "rrrg"}),
    "-force_alpha": (0, lambda: {"force_alpha": True}),
    "-no_alpha": (0, lambda: {"check_for_alpha": False}),
    "-y_flip": (0, lambda: {"y_flip": True}),
    "-resample": (2, lambda w, h: {"resample": (int(w), int(h))}),
    "-resample_factor": (1, lambda f: {"resample": float(f)}),
    "-mipmap": (0, lambda: {"mipmaps": True}),
    "-mip_filter": (1, lambda f: {"mip_filter": f}),
    "-mip_scale": (1, lambda s: {"mip_scale": float(s)}),
    "-mip_clamp": (0, lambda: {"mip_wrapping": False}),
    "-mip_linear": (0, lambda: {"mip_srgb": False}),
    "-mip_renorm": (0, lambda: {"mip_renormalize": True}),
    "-mip_slow": (0, lambda: {"mip_fast": False}),
    "-mip_smallest": (1, lambda n: {"mip_smallest_dimension": int(n)}),
    "-no_selector_rdo": (0, lambda: {"no_selector_rdo": True}),
    "-no_endpoint_rdo": (0, lambda: {"no_endpoint_rdo": True}),
}


def kwargs_from_flags(flags, normal_map_options=None):
    """the tool's flags of a case -> keyword arguments of compress(); `-normal_map` expands to normal_map_options() (basis_universal_amd.source), passed in so that this
    module does not need the package"""
    out, at = {}, 0
    while at < len(flags):
        flag = flags[at]
        if flag == "-normal_map":
            out.update(normal_map_options())
            at += 1
            continue
        count, make = _FLAGS[flag]
        out.update(make(*flags[at + 1:at + 1 + count]))
        at += 1 + count
    return out


PREPARE_KEYS = ("renormalize", "swizzle", "check_for_alpha", "force_alpha", "y_flip")


def prepare_kwargs(kw):
    """the part of a case's keyword arguments that the per-pixel pass takes"""
    return {k: v for k, v in kw.items() if k in PREPARE_KEYS}


def codec_kwargs(case):
    return {"uastc": True, "ktx2": case["ext"] == "ktx2"} if case["uastc"] else {"quality": 128, "ktx2": case["ext"] == "ktx2"}


# ---------------------------------------------------------------- the 2^24 colours

def all_colours_image():
    """4096 x 4096: pixel i = y * 4096 + x has r = i & 255, g = (i >> 8) & 255, b = i >> 16 -- every RGB value once -- and alpha = (5 x + 3 y + (x ^ y)) & 255"""
    i = np.arange(ALL_SIDE * ALL_SIDE, dtype=np.uint32)
    x, y = i % ALL_SIDE, i // ALL_SIDE
    px = i | (((5 * x + 3 * y + (x ^ y)) & 255) << 24)
    return px.view(np.uint8).reshape(ALL_SIDE, ALL_SIDE, 4)


def band_digests(raster):
    """(4096, 4096, 4) u8 -> the SHA-256 of every band of 64 rows"""
    assert raster.shape == (ALL_SIDE, ALL_SIDE, 4) and raster.dtype == np.uint8
    return [hashlib.sha256(np.ascontiguousarray(raster[at:at + BAND_ROWS]).tobytes()).hexdigest() for at in range(0, ALL_SIDE, BAND_ROWS)]


# ---------------------------------------------------------------- the golden files and the host build

@functools.lru_cache(maxsize=None)
def golden():
    """-> (arrays, meta) of source_prep_vectors.npz: loaded once and shared; nobody writes into the arrays"""
    return native_libs.load_npz_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def digests():
    return json.loads(DIGESTS.read_text())


def golden_cases():
    return golden()[1]["cases"]


def slices_of(case):
    """the tool's prepared rasters of a case, one per slice, padded to whole blocks as the tool pads them"""
    return [golden()[0][f"slice{k}_{case['name']}"] for k in range(case["slices"])]


def host():
    return native_libs.load("source_prep_host")


def host_renormalize(img):
    out = np.array(img, np.uint8, order="C")
    host().sph_renormalize(out.ctypes.data, out.size // 4)
    return out


def pack_swizzle(swizzle):
    """None / four of "rgba0123" / four ints -> the packed word (valid input only: the package's own parser is what the tests check for refusals)"""
    if swizzle is None:
        return 0x03020100
    entries = ["rgba".index(c.lower()) if c.lower() in "rgba" else int(c) for c in swizzle] if isinstance(swizzle, str) else list(swizzle)
    return sum(int(e) << (8 * k) for k, e in enumerate(entries))


def host_prepare(img, renormalize=False, swizzle=None, check_for_alpha=True, force_alpha=False, y_flip=False):
    """-> (prepared (h, w, 4) u8, has_alpha, any prepared alpha below 255)"""
    src = np.ascontiguousarray(img, np.uint8)
    h, w = src.shape[:2]
    dst, flags = np.zeros_like(src), np.zeros(2, np.uint32)
    assert host().sph_prepare(src.ctypes.data, w, h, w, dst.ctypes.data, w, int(renormalize), pack_swizzle(swizzle), int(check_for_alpha), int(force_alpha), int(y_flip),
                              flags.ctypes.data) == 1
    return dst, bool(flags[0]), bool(flags[1])


def host_split_alpha(img):
    src = np.ascontiguousarray(img, np.uint8)
    rgb, alpha = np.zeros_like(src), np.zeros_like(src)
    host().sph_split_alpha(src.ctypes.data, src.size // 4, rgb.ctypes.data, alpha.ctypes.data)
    return rgb, alpha
