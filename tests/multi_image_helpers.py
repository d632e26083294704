"""The cases of tests/golden/multi_image_vectors.npz: several source images in one file, compressed by the reference tool (tools/gen_golden_multi_image.py) and by
compress(). One table for the generator and the tests: per case the images, the tool's arguments and the keyword arguments of compress() that say the same."""
import json
import pathlib
import re

import numpy as np

import helpers

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "multi_image_vectors.npz"
SLICE_LINE = re.compile(r"Slice: (\d+), alpha: (\d+), orig width/height: (\d+)x(\d+), width/height: (\d+)x(\d+), first_block: (\d+), image_index: (\d+), mip_level: (\d+), iframe: (\d+)")
SLICE_FIELDS = ("slice", "alpha", "orig_width", "orig_height", "width", "height", "first_block", "image", "level", "iframe")


def alpha_ramp(img):
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    out = img.copy()
    out[..., 3] = np.clip(40 + xx * 9 + yy * 4, 0, 255).astype(np.uint8)
    return out


def _faces():
    faces = [helpers.synth(16, 16, 400 + i) for i in range(6)]
    faces[3] = alpha_ramp(faces[3])
    return faces


def _frames():
    base = helpers.synth(16, 16, 420)
    frames = []
    for f in range(4):
        img = base.copy()
        img[4:12, 2 * f:2 * f + 8] = helpers.synth(8, 8, 430 + f)
        frames.append(img)
    frames[3] = alpha_ramp(frames[3])
    return frames


def cases():
    """name -> {"images", "tool": the tool's arguments, "kw": compress()'s}; every case is compressed into both containers (UASTC .ktx2 without Zstandard)"""
    etc1s, uastc = ["-q", "128", "-comp_level", "1"], ["-uastc", "-ktx2_no_zstandard"]
    return {
        "a_etc1s_array_mips": dict(images=[helpers.synth(16, 16, 440 + i) for i in range(3)], tool=[*etc1s, "-tex_type", "2darray", "-mipmap"],
                                   kw=dict(tex_type="2darray", mipmaps=True)),
        "b_etc1s_cubemap_alpha": dict(images=_faces(), tool=[*etc1s, "-tex_type", "cubemap"], kw=dict(tex_type="cubemap")),
        "c_uastc_cubemap_alpha": dict(images=_faces(), tool=[*uastc, "-tex_type", "cubemap"], kw=dict(tex_type="cubemap", uastc=True)),
        "d_etc1s_video_alpha": dict(images=_frames(), tool=[*etc1s, "-tex_type", "video"], kw=dict(tex_type="video")),
        "e_uastc_video": dict(images=_frames(), tool=[*uastc, "-tex_type", "video"], kw=dict(tex_type="video", uastc=True)),
        "f_uastc_array_ragged_mips_rdo": dict(images=[np.ascontiguousarray(helpers.synth(20, 28, 450 + i)) for i in range(2)],
                                              tool=[*uastc, "-tex_type", "2darray", "-mipmap", "-uastc_rdo_l", "1"],
                                              kw=dict(tex_type="2darray", uastc=True, mipmaps=True, uastc_rdo_lambda=1.0)),
        "g_etc1s_volume": dict(images=[helpers.synth(16, 16, 460 + i) for i in range(2)], tool=[*etc1s, "-tex_type", "3d"], kw=dict(tex_type="volume")),
        "h_etc1s_array_mips_level2": dict(images=[helpers.synth(16, 16, 470 + i) for i in range(2)], tool=["-q", "128", "-comp_level", "2", "-tex_type", "2darray", "-mipmap"],
                                          kw=dict(tex_type="2darray", mipmaps=True, comp_level=2)),
    }


def refusals():
    """name -> (images, the tool's arguments): what the tool refuses, by exit status"""
    small, other = helpers.synth(16, 16, 480), np.ascontiguousarray(helpers.synth(20, 28, 481))
    return {
        "array_of_two_sizes": ([small, other], ["-q", "128", "-tex_type", "2darray"]),
        "cubemap_of_five": ([helpers.synth(16, 16, 482 + i) for i in range(5)], ["-q", "128", "-tex_type", "cubemap"]),
        "two_files_as_2d": ([small, helpers.synth(16, 16, 488)], ["-q", "128", "-tex_type", "2d"]),
    }


def load():
    """-> (npz, meta): file_<case>_<basis|ktx2>, image_<case>_<i>, slices_<case> (one row of SLICE_FIELDS per slice, as the tool printed them), meta["refusals"]"""
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta"]).decode())


def golden_images(g, name):
    out, i = [], 0
    while f"image_{name}_{i}" in g.files:
        out.append(g[f"image_{name}_{i}"])
        i += 1
    return out


class Untouchable:
    """a context stand-in for refusals that must come before any device work: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were refused")
