"""The cases of tests/golden/mip_levels_vectors.npz: .dds sources whose mip chains the reference tool used as they are (tools/gen_golden_mip_levels.py), compressed
again by compress(mip_levels=) and dds.compress_dds. One table for the generator and the tests: per case the files' levels, the tool's arguments and the keyword
arguments of compress() that say the same. Every level of every file is an independent helpers.synth image, so a chain that was GENERATED from level 0 cannot give
the tool's file by accident. Also the .dds writers of the tests (DX10 and legacy headers, both byte orders) and the numpy statement of what a supplied level becomes."""
import json
import pathlib
import struct

import numpy as np

import helpers
from basis_universal_amd import dds

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "mip_levels_vectors.npz"
READ_LINE = r'Read DDS file "in(\d+)\.dds", LDR, (\d+)x(\d+), (\d+) mipmap levels'
ORDERS = {"rgba": [0, 1, 2, 3], "bgra": [2, 1, 0, 3]}
LEGACY_MASKS = {"rgba": (0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000), "bgra": (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000)}


def level_image(w, h, seed):
    """helpers.synth of any size: made at the next multiple of four and cropped"""
    return np.ascontiguousarray(helpers.synth((w + 3) // 4 * 4, (h + 3) // 4 * 4, seed)[:h, :w])


def chain(w, h, n_levels, seed, alpha_level=None):
    """n_levels independent images, level k max(1, w >> k) x max(1, h >> k); alpha_level: that level alone gets alpha values below 255"""
    out = []
    for k in range(n_levels):
        img = level_image(max(1, w >> k), max(1, h >> k), seed + k)
        if k == alpha_level:
            yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
            img[..., 3] = np.clip(60 + xx * 31 + yy * 17, 0, 254).astype(np.uint8)
        out.append(img)
    return out


def legacy_header(width, height, levels, order):
    """a DDS_HEADER without the DX10 extension: 32 bits per pixel, DDPF_RGB | DDPF_ALPHAPIXELS, the masks of A8B8G8R8 ("rgba") or A8R8G8B8 ("bgra")"""
    flags = 0x1 | 0x2 | 0x4 | 0x8 | 0x1000 | (0x20000 if levels > 1 else 0)
    caps = 0x1000 | (0x8 | 0x400000 if levels > 1 else 0)
    head = struct.pack("<4s7I44x", b"DDS ", 124, flags, height, width, width * 4, 0, levels)
    head += struct.pack("<8I", 32, 0x41, 0, 32, *LEGACY_MASKS[order])
    head += struct.pack("<5I", caps, 0, 0, 0, 0)
    assert len(head) == 128
    return head


def dds_file(levels, order="rgba", srgb=False, legacy=False, mip_count=None):
    """levels: RGBA arrays, level 0 first -> the bytes of a 2D .dds file that holds them in `order`"""
    h, w = levels[0].shape[:2]
    n = len(levels) if mip_count is None else mip_count
    head = legacy_header(w, h, n, order) if legacy else dds.dds_header(w, h, n, 1, False, "a8b8g8r8" if order == "rgba" else "a8r8g8b8", srgb)
    return np.frombuffer(head + b"".join(np.ascontiguousarray(lv[..., ORDERS[order]]).tobytes() for lv in levels), np.uint8).copy()


def swizzled(level, swizzle):
    """what the reference makes of a supplied level: the swizzle and nothing else (comp.cpp:2796-2817)"""
    letters = {"r": 0, "g": 1, "b": 2, "a": 3}
    return np.ascontiguousarray(level[..., [letters[c] for c in swizzle]]) if swizzle else level


def cases():
    """name -> {"files": per file dict(levels=[RGBA arrays], order, srgb, legacy), "tool": the tool's arguments, "kw": compress()'s, "exts": the containers written,
    "slices": the tool's slice count, "alpha": the alpha flag of every slice in order, "stats": record the tool's -stats figures}"""
    etc1s, uastc = ["-q", "128", "-comp_level", "1"], ["-uastc", "-ktx2_no_zstandard"]

    def one(levels, order="rgba", srgb=False, legacy=False):
        return dict(levels=levels, order=order, srgb=srgb, legacy=legacy)
    alpha3 = chain(20, 28, 3, 620, alpha_level=2)
    pair = [one(chain(16, 16, 3, 700)), one(chain(16, 16, 3, 710, alpha_level=1), order="bgra")]
    return {
        "a_etc1s_full_chain": dict(files=[one(chain(20, 28, 5, 600), srgb=True)], tool=etc1s, kw={}, exts=("basis", "ktx2"), slices=5, alpha=[0] * 5, stats=True),
        "b_etc1s_three_levels": dict(files=[one(chain(20, 28, 3, 610), order="bgra")], tool=etc1s, kw={}, exts=("basis", "ktx2"), slices=3, alpha=[0] * 3),
        "c_etc1s_alpha_in_level_2": dict(files=[one(alpha3, order="bgra", srgb=True)], tool=etc1s, kw={}, exts=("basis",), slices=6, alpha=[0, 1] * 3),
        "d_etc1s_alpha_in_level_2_no_alpha": dict(files=[one(alpha3)], tool=[*etc1s, "-no_alpha"], kw=dict(check_for_alpha=False), exts=("basis",), slices=6,
                                                  alpha=[0, 1] * 3),
        "e_uastc_alpha_in_level_2": dict(files=[one(alpha3)], tool=uastc, kw=dict(uastc=True), exts=("ktx2",), slices=3, alpha=[0, 0, 1], stats=True),
        "f_etc1s_swizzle_rrrg": dict(files=[one(chain(20, 28, 3, 630))], tool=[*etc1s, "-swizzle", "rrrg"], kw=dict(swizzle="rrrg"), exts=("basis",), slices=6,
                                     alpha=[0, 1] * 3),
        "g_etc1s_y_flip_renorm": dict(files=[one(chain(20, 28, 3, 640))], tool=[*etc1s, "-y_flip", "-renorm"], kw=dict(y_flip=True, renormalize=True), exts=("basis",),
                                      slices=3, alpha=[0] * 3),
        "h_etc1s_mipmap_ignored": dict(files=[one(chain(20, 28, 3, 650))], tool=[*etc1s, "-mipmap"], kw=dict(mipmaps=True), exts=("basis",), slices=3, alpha=[0] * 3),
        "i_etc1s_legacy_bgra": dict(files=[one(chain(20, 28, 3, 660), order="bgra", legacy=True)], tool=etc1s, kw={}, exts=("basis",), slices=3, alpha=[0] * 3),
        "j_etc1s_legacy_rgba": dict(files=[one(chain(20, 28, 5, 670), legacy=True)], tool=etc1s, kw={}, exts=("basis",), slices=5, alpha=[0] * 5),
        "k_etc1s_array_alpha_in_one_level": dict(files=pair, tool=[*etc1s, "-tex_type", "2darray"], kw=dict(tex_type="2darray"), exts=("basis",), slices=12,
                                                 alpha=[0, 1] * 6),
        "l_uastc_array_alpha_in_one_level": dict(files=pair, tool=[*uastc, "-tex_type", "2darray"], kw=dict(tex_type="2darray", uastc=True), exts=("ktx2",), slices=6,
                                                 alpha=[0, 0, 0, 0, 1, 0]),
    }


def load():
    """-> (npz, meta): dds_<case>_<i> (the source files), file_<case>_<basis|ktx2>, slices_<case> (multi_image_helpers.SLICE_FIELDS rows, as the tool printed them),
    stats_<case> (image_stats_vectors.npz's layout: (slices, 8 lines, 4 figures)) for the cases with stats"""
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta"]).decode())


def golden_sources(g, name):
    out, i = [], 0
    while f"dds_{name}_{i}" in g.files:
        out.append(g[f"dds_{name}_{i}"])
        i += 1
    return out


def rgba_levels(parsed):
    """dds.read_dds_source's result -> the levels as RGBA arrays, by numpy"""
    order = ORDERS[parsed["byte_order"]]
    return [np.ascontiguousarray(parsed["payload"][lv["offset"]:lv["offset"] + lv["nbytes"]].reshape(lv["height"], lv["width"], 4)[..., order]) for lv in parsed["levels"]]
