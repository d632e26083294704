#!/usr/bin/env python3
"""The source side of compress() with several images, measured on the device: resident level-0 rasters -> resident tiles of every slice, once with the batched
kernel (bu_hip_k_extract_slices: the mip launches, then ONE launch for every slice) and once the way the single-image path does it per image and level
(split_alpha + an allocation, then k_extract_blocks per slice), alternating; the same two from resident LEVELS (the tiling alone, without the mip launches both
sides share); plus the whole compress() call and the launch counts of both.

Workloads: `video` -- 64 frames of 256x256 with alpha, ETC1S video (128 slices); `cubemap` -- six 1024x1024 faces with mips, UASTC (66 slices).
Times are host clock around work that ends in a stream synchronise, after warm-up; per side the median and the extremes of --repeats rounds.
The launch counts come from a separate profiled pass (bu_hip_profile_*), not from the timed rounds. One JSON line per workload.
usage: multi_image_bench.py [--workload video|cubemap|all] [--repeats N] [--out FILE]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import helpers  # noqa: E402
from basis_universal_amd import capi, mipmap, source  # noqa: E402
from basis_universal_amd.compress import compress  # noqa: E402


def workloads():
    def video():
        base = helpers.synth(256, 256, 900)
        yy, xx = np.mgrid[0:256, 0:256]
        base[..., 3] = np.clip(128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 13.0), 0, 255).astype(np.uint8)
        frames = []
        for f in range(64):
            img = base.copy()
            img[64:128, 2 * f:2 * f + 96, :3] = helpers.synth(96, 64, 901)[..., :3]
            frames.append(img)
        return frames, dict(tex_type="video"), False

    def cubemap():
        return [helpers.synth(1024, 1024, 910 + i) for i in range(6)], dict(tex_type="cubemap", uastc=True, mipmaps=True), True
    return {"video": video, "cubemap": cubemap}


class Resident:
    """the level-0 rasters of a workload, resident, and what both sides need to know about its slices"""

    def __init__(self, ctx, images, uastc, mipmaps):
        self.ctx, self.uastc = ctx, uastc
        self.any_alpha = any(bool((img[..., 3] != 255).any()) for img in images)
        w, h = images[0].shape[1], images[0].shape[0]
        self.levels = [(w, h)] + (mipmap.level_sizes(w, h, 1) if mipmaps else [])
        self.slices, self.sources = source.slice_table([self.levels] * len(images), uastc=uastc, any_alpha=self.any_alpha, image_alpha=[self.any_alpha] * len(images))
        self.total = sum(s[1] * s[2] for s in self.slices)
        self.d_tiles = ctx.alloc(self.total * 64)
        # every level's buffer is allocated once, so that neither side pays for it; the per-slice side splits alpha IN PLACE (as compress() does for one image), so it
        # works on a copy of level 0 that is restored outside the timed part (restore_copies)
        self.chains = [[ctx.upload(np.ascontiguousarray(img))] + [ctx.alloc(lw * lh * 4) for lw, lh in self.levels[1:]] for img in images]
        self.copies = [[ctx.alloc(lw * lh * 4) for lw, lh in self.levels] for _ in images]
        self.make_levels(self.chains)
        self.restore_copies()

    def restore_copies(self):
        for chain, copy in zip(self.chains, self.copies):
            for d_src, d_dst, (lw, lh) in zip(chain, copy, self.levels):
                self.ctx.memcpy_d2d(d_dst, d_src, lw * lh * 4)
        self.ctx.sync()

    def make_levels(self, chains):
        ctx = self.ctx
        for chain in chains:
            for at, (lw, lh) in enumerate(self.levels[1:]):
                sw, sh = self.levels[at]
                ctx.check(mipmap._lib().bu_generate_mipmap_level(ctx.h, chain[at], sw, sh, chain[at + 1], lw, lh, 1, b"kaiser", 1.0, 1, 4 if self.any_alpha else 3),
                          "bu_generate_mipmap_level")

    def batched(self, levels=True):
        if levels:
            self.make_levels(self.chains)
        entries = [(self.chains[k][level], s[3], s[4], 0, mode, s[0]) for s, (k, level, mode) in zip(self.slices, self.sources)]
        source.extract_slices_resident(self.ctx, entries, self.d_tiles)
        self.ctx.sync()

    def per_slice(self, levels=True):
        """what compress() does for ONE image, here per image: per level split_alpha into the level's own buffer and a newly allocated alpha plane, then
        k_extract_blocks per plane"""
        ctx, split, planes_owned, first = self.ctx, self.any_alpha and not self.uastc, [], 0
        if levels:
            self.make_levels(self.copies)
        for chain in self.copies:
            for d_raster, (lw, lh) in zip(chain, self.levels):
                planes = [d_raster]
                if split:
                    planes.append(ctx.alloc(lw * lh * 4))
                    planes_owned.append(planes[1])
                    source.split_alpha_resident(ctx, d_raster, lw, lh, planes[0], planes[1])
                for d_plane in planes:
                    ctx.check(ctx.lib.k_extract_blocks(ctx.h, d_plane, lw, lh, lw * 4, self.d_tiles + first * 64), "k_extract_blocks")
                    first += ((lw + 3) // 4) * ((lh + 3) // 4)
        ctx.sync()
        for d in planes_owned:
            ctx.free(d)

    def tiles(self):
        return self.ctx.download(self.d_tiles, (self.total, 64), np.uint8)

    def close(self):
        for d in [self.d_tiles] + [d for chain in self.chains + self.copies for d in chain]:
            self.ctx.free(d)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def launches(ctx, fn):
    ctx.profile_enable(True)
    fn()
    counts = {k: n for k, (_, n) in ctx.profile_read().items()}
    ctx.profile_enable(False)
    return counts


def run(ctx, name, make, repeats):
    images, kw, _ = make()
    res = Resident(ctx, images, bool(kw.get("uastc")), bool(kw.get("mipmaps")))
    try:
        res.per_slice()
        expected = res.tiles()
        res.batched()
        same = bool((res.tiles() == expected).all())          # faster and different is not faster
        for _ in range(3):                                    # warm-up of both sides
            res.batched()
            res.restore_copies()
            res.per_slice()
        a, b, a_tiles, b_tiles = [], [], [], []
        for _ in range(repeats):                              # alternating, so that both sides see the same machine
            a.append(timed(res.batched))
            res.restore_copies()
            b.append(timed(res.per_slice))
            a_tiles.append(timed(lambda: res.batched(levels=False)))       # the levels are resident already: the tiling alone
            res.restore_copies()
            b_tiles.append(timed(lambda: res.per_slice(levels=False)))
        count_a = launches(ctx, res.batched)
        res.restore_copies()
        count_b = launches(ctx, res.per_slice)
        compress(ctx, images, **kw)                           # warm-up of the whole call
        whole = [timed(lambda: compress(ctx, images, **kw)) for _ in range(3)]
        return {"workload": name, "images": len(images), "size": list(images[0].shape[1::-1]), "slices": len(res.slices), "blocks": res.total, "tiles_identical": same,
                "rasters_to_tiles_batched": summary(a), "rasters_to_tiles_per_slice": summary(b), "levels_to_tiles_batched": summary(a_tiles),
                "levels_to_tiles_per_slice": summary(b_tiles), "launches_batched": count_a, "launches_per_slice": count_b,
                "compress_call": summary(whole), "repeats": repeats}
    finally:
        res.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["video", "cubemap", "all"])
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = capi.Context(0)       # no device, no numbers: this raises
    lines = []
    for name, make in workloads().items():
        if args.workload in ("all", name):
            lines.append(json.dumps(run(ctx, name, make, args.repeats)))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")
