"""Mip generation on the device: basis_compressor::generate_mipmaps (encoder/basisu_comp.cpp:2146-2230) as a chain of
bu_generate_mipmap_level calls -- contributor lists on the host exactly as the reference's Resampler builds them, pixels resampled by the HIP
kernels of mipmap_kernels.hip. Byte-identical to image_resample, its shortcut included: equal sizes at filter scale 1 copy the source, all four channels."""
import ctypes as C

import numpy as np

from . import capi, source
from .etc1s import load_frontend_library

_vp = C.c_void_p


_lib = load_frontend_library   # bench.py reaches for this name


def level_sizes(w, h, smallest_dimension=1):
    out = np.zeros(64, np.uint32)
    n = _lib().bu_mipmap_level_sizes(w, h, smallest_dimension, out.ctypes.data_as(_vp), 32)
    return [tuple(int(v) for v in out[2 * i:2 * i + 2]) for i in range(n)]


def resample(ctx, image, dst_w, dst_h, srgb=True, filter="kaiser", filter_scale=1.0, wrapping=True, num_comps=4):
    """image_resample on the GPU: (h, w, 4) u8 -> (dst_h, dst_w, 4) u8."""
    img = np.ascontiguousarray(image, np.uint8)
    h, w = img.shape[:2]
    d_src, d_dst = ctx.upload(img), ctx.alloc(dst_w * dst_h * 4)
    try:
        ctx.check(_lib().bu_generate_mipmap_level(ctx.h, d_src, w, h, d_dst, dst_w, dst_h, int(srgb), filter.encode(), filter_scale, int(wrapping), num_comps),
                  "bu_generate_mipmap_level")
        return ctx.download(d_dst, (dst_h, dst_w, 4), np.uint8)
    finally:
        ctx.free(d_src); ctx.free(d_dst)


def generate_mipmaps(ctx, image, has_alpha=False, srgb=True, filter="kaiser", filter_scale=1.0, wrapping=True, smallest_dimension=1, fast=True):
    """The levels below `image` ((h, w, 4) u8) with the compressor's defaults; with `fast` (m_mip_fast) every level past the first is made from
    the one above it, all on the device: one upload, one download per level."""
    img = np.ascontiguousarray(image, np.uint8)
    h, w = img.shape[:2]
    sizes = [(w, h)] + level_sizes(w, h, smallest_dimension)
    owned = [ctx.upload(img)]
    try:
        chain = resident_chain(ctx, owned, owned[0], sizes, srgb=srgb, filter=filter, filter_scale=filter_scale, wrapping=wrapping, num_comps=4 if has_alpha else 3, fast=fast)
        return [ctx.download(d, (lh, lw, 4), np.uint8) for d, (lw, lh) in zip(chain[1:], sizes[1:])]
    finally:
        for d in owned:
            ctx.free(d)


def resident_chain(ctx, owned, d_level0, sizes, *, srgb=True, filter="kaiser", filter_scale=1.0, wrapping=True, num_comps=4, fast=True, renormalize=False):
    """The mip chain of a resident level 0, resident: sizes = the (width, height) of level 0 and of every level below it (level_sizes). With `fast` (m_mip_fast) every
    level is made from the one above it, else from level 0; `renormalize` (m_mip_renormalize): every level renormalised after it is made. What is allocated here is
    appended to the caller's `owned`, level by level, so that a failure half way leaks nothing. -> [d_level0, d_level1, ...]; no synchronisation."""
    chain = [d_level0]
    for lw, lh in sizes[1:]:
        d = ctx.alloc(lw * lh * 4)
        owned.append(d)
        at = len(chain) - 1 if fast else 0
        sw, sh = sizes[at]
        ctx.check(_lib().bu_generate_mipmap_level(ctx.h, chain[at], sw, sh, d, lw, lh, int(bool(srgb)), filter.encode(), float(filter_scale), int(bool(wrapping)), num_comps),
                  "bu_generate_mipmap_level")
        if renormalize:
            source.renormalize_resident(ctx, d, lw, lh)
        chain.append(d)
    return chain
