#!/usr/bin/env python3
"""Known answers of the block unpacker from the real reference (oracle/_ref/libref_harness.so, build machine only) -> tests/golden/block_unpack_vectors.npz.

The reference's answer is basisu::unpack_block(texture_format, const void*, color_rgba*, bool) (encoder/basisu_gpu_texture.cpp:984), which the harness library exports
because it links basisu_gpu_texture.o with default visibility: called through ctypes, one block at a time, into 16 texels pre-filled with (0, 0, 0, 255) as
gpu_image::unpack pre-fills them. Per member `<name>_blocks` (n, 8 | 16) u8, `<name>_texels` (n, 16, 4) u8 as the reference left them (for a BC7 block it refuses:
the pre-fill) and `<name>_ok` (n,) u8, its return value. Everything from one fixed seed through PCG64's raw stream.

  bc7   coverage by construction: per mode the mode prefix is fixed and every other bit random, then the field that follows the prefix is set -- modes 1, 2, 3, 7:
        8 blocks for each of the 64 partitions; mode 0: 8 for each of its 16; mode 4: 32 for each of the 8 (rotation, index selection) settings; mode 5: 32 for
        each of the 4 rotations; mode 6: 256 -- then per mode 4 blocks with every endpoint and p-bit 0 and 4 with every one 1, then 16 blocks with byte 0 == 0.
  bc1   256 random; 64 each with low > high, low < high, low == high (forced by swapping / copying), each group using index 3.
  bc4   256 random; 64 each of low > high, low < high, low == high, with (0, 255) and (255, 0) among them.
  bc3   256 random; 64 whose colour half has low <= high (decoded with four colours all the same).   bc5   256 random.
  level2_{bc1,bc1_hq,bc3,bc4_r,bc5_ra,bc7}: the first 512 blocks of those arrays of tests/golden/uastc_transcode_vectors.npz -- what this package's transcoders write.
`meta` records the counts; tests/test_block_unpack_host.py re-derives them from the blocks.
usage: gen_golden_block_unpack.py"""
import ctypes as C
import json
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import block_unpack_helpers as B  # noqa: E402
import gen_golden_image_stats as S  # noqa: E402

HARNESS = ROOT / "oracle" / "_ref" / "libref_harness.so"
SEED = 20261018
REF_FORMAT = {B.BC1: 5, B.BC3: 6, B.BC4: 7, B.BC5: 8, B.BC7: 11}   # basisu::texture_format (transcoder/basisu.h:513)
ENCODER_MADE_BLOCKS = 512


class Bits:
    """The raw 64-bit stream of PCG64: the one part of numpy's random module whose output for a seed is promised not to change."""

    def __init__(self, seed):
        self.g = np.random.PCG64(seed)

    def blocks(self, n, size):
        return self.g.random_raw(n * size // 8).astype("<u8").view(np.uint8).reshape(n, size).copy()


def reference_unpack():
    assert HARNESS.exists(), "oracle/_ref/libref_harness.so is missing: build it on the build machine (make -C oracle ref)"
    names = subprocess.run(["nm", "-DC", str(HARNESS)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    want = "basisu::unpack_block(basisu::texture_format, void const*, basisu::color_rgba*, bool)"
    at = [k for k, line in enumerate(names) if line.endswith(" T " + want)]
    assert len(at) == 1, f"the harness does not export {want}"
    mangled = subprocess.run(["nm", "-D", str(HARNESS)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()[at[0]].split()[-1]
    fn = getattr(C.CDLL(str(HARNESS)), mangled)
    fn.restype = C.c_bool
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_bool]

    def unpack(blocks, fmt):
        blocks = np.ascontiguousarray(blocks, np.uint8)
        n = blocks.shape[0]
        texels, ok = np.zeros((n, 16, 4), np.uint8), np.zeros(n, np.uint8)
        texels[..., 3] = 255
        for i in range(n):
            ok[i] = 1 if fn(REF_FORMAT[fmt], blocks[i].ctypes.data, texels[i].ctypes.data, False) else 0
        return texels, ok
    return unpack


def put(blocks, ofs, width, value):
    """write `value` into bits ofs .. ofs + width of every block (little-endian bit order)"""
    for b in blocks:
        v = int.from_bytes(b.tobytes(), "little")
        mask = ((1 << width) - 1) << ofs
        v = (v & ~mask) | ((int(value) << ofs) & mask)
        b[:] = np.frombuffer(v.to_bytes(b.size, "little"), np.uint8)


def bc7_blocks(rng):
    out, counts = [], {}
    for mode in range(8):
        if mode in B.BC7_PARTITION_BITS:
            settings, per, ofs, width = 1 << B.BC7_PARTITION_BITS[mode], 8, mode + 1, B.BC7_PARTITION_BITS[mode]
        elif mode == 4:
            settings, per, ofs, width = 8, 32, 5, 3
        elif mode == 5:
            settings, per, ofs, width = 4, 32, 6, 2
        else:
            settings, per, ofs, width = 1, 256, 7, 0
        for s in range(settings):
            blk = rng.blocks(per, 16)
            put(blk, 0, mode + 1, 1 << mode)
            if width:
                put(blk, ofs, width, s)
            out.append(blk)
        first, length = B.BC7_ENDPOINT_FIELDS[mode]
        for fill in (0, (1 << length) - 1):
            blk = rng.blocks(4, 16)
            put(blk, 0, mode + 1, 1 << mode)
            put(blk, first, length, fill)
            out.append(blk)
        counts[str(mode)] = settings * per + 8
    bad = rng.blocks(16, 16)
    bad[:, 0] = 0
    out.append(bad)
    counts["reserved"] = 16
    return np.concatenate(out), counts


def ordered_pairs(rng, size, lo_at, width, extremes):
    """64 blocks each with low > high, low < high, low == high, where the two endpoints are `width` bits at bit lo_at and lo_at + width"""
    groups = []
    for order in (">", "<", "="):
        blk = rng.blocks(64, size)
        for k, b in enumerate(blk):
            lo, hi = B.field(b, lo_at, width), B.field(b, lo_at + width, width)
            if extremes and k == 0 and order != "=":
                lo, hi = (extremes[1], extremes[0]) if order == ">" else extremes
            if lo == hi and order != "=":
                hi = lo ^ 1
            big, small = max(lo, hi), min(lo, hi)
            lo, hi = (big, small) if order == ">" else ((small, big) if order == "<" else (lo, lo))
            put(b[None], lo_at, width, lo)
            put(b[None], lo_at + width, width, hi)
        groups.append(blk)
    return np.concatenate(groups)


def members(rng):
    bc7, counts = bc7_blocks(rng)
    bc1 = np.concatenate([rng.blocks(256, 8), ordered_pairs(rng, 8, 0, 16, None)])
    bc4 = np.concatenate([rng.blocks(256, 8), ordered_pairs(rng, 8, 0, 8, (0, 255))])
    colour = ordered_pairs(rng, 16, 64, 16, None)
    bc3 = np.concatenate([rng.blocks(256, 16), colour[64:96], colour[128:160]])   # 32 with low < high and 32 with low == high in the colour half
    bc5 = rng.blocks(256, 16)
    return {"bc7": (bc7, B.BC7), "bc1": (bc1, B.BC1), "bc4": (bc4, B.BC4), "bc3": (bc3, B.BC3), "bc5": (bc5, B.BC5)}, counts


if __name__ == "__main__":
    unpack = reference_unpack()
    sets, bc7_counts = members(Bits(SEED))
    transcoded = np.load(ROOT / "tests" / "golden" / "uastc_transcode_vectors.npz")
    for name, fmt in B.ENCODER_MADE.items():
        sets[name] = (np.array(transcoded[name][:ENCODER_MADE_BLOCKS]), fmt)
    arrays, meta = {}, {"seed": SEED, "bc7_counts": bc7_counts, "members": {}}
    for name, (blocks, fmt) in sets.items():
        texels, ok = unpack(blocks, fmt)
        arrays[name + "_blocks"], arrays[name + "_texels"], arrays[name + "_ok"] = blocks, texels, ok
        meta["members"][name] = {"format": fmt, "blocks": int(blocks.shape[0]), "refused": int((ok == 0).sum())}
        print(name, blocks.shape, "refused", int((ok == 0).sum()), flush=True)
    B.check_coverage(arrays, meta)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    S.save(B.GOLDEN, arrays)
    assert B.GOLDEN.stat().st_size <= 1 << 20, B.GOLDEN.stat().st_size
    print("wrote", B.GOLDEN, B.GOLDEN.stat().st_size, "bytes,", len(arrays), "members")
