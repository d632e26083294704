"""-m gpu: mip generation on the device against the real image_resample / the reference tool: the HIP kernels apply the
host-built resampling plan (tests/test_mipmap_host.py pins the plan itself on the CPU) and have to write the reference's bytes."""
import numpy as np
import pytest

from helpers import have_ref, have_ref_cli, synth, to_pixel_blocks

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref not present")


@needs_ref
def test_resample_matches_image_resample(hip_ctx):
    from basis_universal_amd import mipmap
    from test_mipmap_host import CASES, rgba, reference
    for sw, sh, dw, dh, srgb, flt, scale, wrap, comps in CASES:
        for seed, noise in ((1, False), (2, True)):
            src = rgba(sw, sh, seed, noise)
            got = mipmap.resample(hip_ctx, src, dw, dh, srgb, flt, scale, wrap, comps)
            exp = reference(src, dw, dh, srgb, flt, scale, wrap, comps)
            assert (got == exp).all(), ((sw, sh, dw, dh, srgb, flt, scale, wrap, comps), np.argwhere(got != exp)[:5])


@needs_ref
@pytest.mark.parametrize("w,h,alpha", [(512, 384, False), (301, 173, True), (1024, 1024, True)])
def test_mip_chain_matches_reference(hip_ctx, w, h, alpha):
    from basis_universal_amd import mipmap
    from test_mipmap_host import rgba
    from test_backend_host import _ref_mip_chain
    img = rgba(w, h, 7)
    if not alpha:
        img[..., 3] = 255
    got = mipmap.generate_mipmaps(hip_ctx, img, has_alpha=alpha)
    exp = _ref_mip_chain(img, alpha)
    assert [g.shape for g in got] == [e.shape for e in exp] and got[-1].shape[:2] == (1, 1)
    for level, (g, e) in enumerate(zip(got, exp)):
        assert (g == e).all(), (level, np.argwhere(g != e)[:5])


GUARD = 0xA5


def _resample_between_guards(ctx, src, case):
    """bu_generate_mipmap_level into the middle of a buffer filled with GUARD, more than a destination row of it in front and behind -> (the raster, the guards intact)"""
    from basis_universal_amd import mipmap
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
    lead, tail = dw + 3, dw + 5
    fill = np.full((lead + dw * dh + tail, 4), GUARD, np.uint8)
    d_src, d_buf = ctx.upload(src), ctx.upload(fill)
    try:
        ctx.check(mipmap._lib().bu_generate_mipmap_level(ctx.h, d_src, sw, sh, d_buf + 4 * lead, dw, dh, int(srgb), flt.encode(), scale, int(wrap), comps), "bu_generate_mipmap_level")
        out = ctx.download(d_buf, fill.shape, np.uint8)
    finally:
        ctx.free(d_src); ctx.free(d_buf)
    return out[lead:lead + dw * dh].reshape(dh, dw, 4), bool((out[:lead] == GUARD).all() and (out[lead + dw * dh:] == GUARD).all())


def _wide_and_magnify():
    from test_mipmap_host import WIDE_AND_MAGNIFY
    return WIDE_AND_MAGNIFY


@pytest.mark.parametrize("case", _wide_and_magnify(), ids=lambda c: "-".join(str(v) for v in c))
def test_resample_matches_the_committed_reference_bytes(hip_ctx, case):
    """the y-first kernels past one workgroup along x, magnification, lists of thousands of taps and the identity copy against tests/golden/resample_vectors.npz (what
    ref_image_resample wrote: needs no oracle/_ref), through mipmap.resample and, between guards, through the C entry point"""
    from basis_universal_amd import mipmap
    from test_mipmap_host import golden, rgba, seeds_of
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
    for seed, noise in seeds_of(case):
        src, exp = rgba(sw, sh, seed, noise), golden()[case, seed]
        got = mipmap.resample(hip_ctx, src, dw, dh, srgb, flt, scale, wrap, comps)
        assert got.shape == exp.shape and (got == exp).all(), (seed, np.argwhere(got != exp)[:5])
        raster, guards_intact = _resample_between_guards(hip_ctx, src, case)
        assert (raster == exp).all(), (seed, np.argwhere(raster != exp)[:5])
        assert guards_intact, seed


def test_resample_scratch_is_reused_across_sizes():
    """the packed lists and the float4 intermediate live in two arenas of the context that grow and are never cleared: the largest case, the smallest, the largest again,
    on a context of their own"""
    from basis_universal_amd import capi, mipmap
    from test_mipmap_host import SEEDS, golden, rgba
    cases = _wide_and_magnify()
    largest = max(cases, key=lambda c: max(c[2] * c[1], c[0] * c[3]))   # the intermediate's pixels, as the launcher sizes it
    smallest = (1, 1, 5, 3, True, "box", 1.0, False, 4)
    assert smallest in cases and largest != smallest
    ctx = capi.Context()
    try:
        for case in (largest, smallest, largest):
            sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
            for seed, noise in SEEDS:
                got = mipmap.resample(ctx, rgba(sw, sh, seed, noise), dw, dh, srgb, flt, scale, wrap, comps)
                assert (got == golden()[case, seed]).all(), (case, seed)
    finally:
        ctx.close()


def test_mip_slow_chain_matches_the_emulation_from_level_0(hip_ctx):
    """-mip_slow: every level of 260x9 is made from level 0 (lists up to 260 x 6 taps long, y first for the upper levels), and has to equal the float32 emulation of the
    plan applied to level 0 -- and, where oracle/_ref is there, image_resample applied to level 0. test_backend_host._ref_mip_chain offers no slow mode (it makes each
    level from the one before), so it is not what this chain is compared with."""
    from basis_universal_amd import mipmap
    from test_mipmap_host import emulate, plan, reference, rgba
    img = rgba(260, 9, 2, True)
    sizes = mipmap.level_sizes(260, 9)
    assert sizes == [(130, 4), (65, 2), (32, 1), (16, 1), (8, 1), (4, 1), (2, 1), (1, 1)]
    got = mipmap.generate_mipmaps(hip_ctx, img, has_alpha=True, fast=False)
    assert [g.shape for g in got] == [(lh, lw, 4) for lw, lh in sizes]
    for level, (g, (lw, lh)) in enumerate(zip(got, sizes), 1):
        exp = emulate(img, lw, lh, plan(260, 9, lw, lh, True, "kaiser", 1.0, True), True, 4)
        assert (g == exp).all(), (level, np.argwhere(g != exp)[:5])
        if have_ref():
            assert (g == reference(img, lw, lh, True, "kaiser", 1.0, True, 4)).all(), level


def test_a_refused_resample_raises_with_the_reason(hip_ctx):
    """the text is this call's, not what an earlier failure left in the context; an unknown filter is not looked at where the sizes are equal at scale 1 (a copy)"""
    from basis_universal_amd import capi, mipmap
    from test_mipmap_host import REFUSED, rgba
    src = rgba(8, 2, 1)
    with pytest.raises(capi.HipError, match='bu_generate_mipmap_level: unknown filter "gauss"'):
        mipmap.resample(hip_ctx, src, 4, 1, filter="gauss")
    with pytest.raises(capi.HipError, match="bu_generate_mipmap_level: destination size 16385x2 is outside 1..16384"):
        mipmap.resample(hip_ctx, src, 16385, 2, filter="box")
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = REFUSED
    with pytest.raises(capi.HipError, match="bu_generate_mipmap_level: filter scale .* without contributors"):
        mipmap.resample(hip_ctx, rgba(sw, sh, 1), dw, dh, srgb, flt, scale, wrap, comps)
    assert (mipmap.resample(hip_ctx, src, 8, 2, filter="gauss", num_comps=3) == src).all()


@pytest.mark.skipif(not have_ref_cli(), reason="oracle/_ref/basisu not present")
@pytest.mark.parametrize("w,h,alpha", [(256, 192, False), (100, 60, True)])
def test_mipmapped_encode_matches_reference_command_line(hip_ctx, tmp_path, w, h, alpha):
    """`basisu -etc1s -q 128 -mipmap x.png`, .basis and .ktx2, against: mips on the device -> tiles -> resident frontend -> backend -> writers."""
    from helpers import save_png, run_ref_cli, basis_file_key_values, ktx2_file_key_values
    from basis_universal_amd import mipmap
    from basis_universal_amd.etc1s import Etc1sFrontend, quality_to_clusters
    from basis_universal_amd.backend import Etc1sBackend, default_params
    img = np.ascontiguousarray(synth((w + 3) // 4 * 4, (h + 3) // 4 * 4, 91)[:h, :w])
    if alpha:
        yy, xx = np.mgrid[0:h, 0:w]
        img[..., 3] = np.clip(128 + 100 * np.sin(xx / 13.0) * np.cos(yy / 11.0), 0, 255).astype(np.uint8)
    save_png(tmp_path / "x.png", img)
    levels = [img] + mipmap.generate_mipmaps(hip_ctx, img, has_alpha=alpha)
    blocks, slices, first = [], [], 0
    for mip, lv in enumerate(levels):
        lh, lw = lv.shape[:2]
        nbx, nby = (lw + 3) // 4, (lh + 3) // 4
        planes = [lv]
        if alpha:
            rgb = lv.copy(); rgb[..., 3] = 255
            a = np.repeat(lv[..., 3:4], 4, axis=2); a[..., 3] = 255
            planes = [rgb, a]
        for k, pl in enumerate(planes):
            blocks.append(to_pixel_blocks(pl))
            slices.append((first, nbx, nby, lw, lh, 0, mip, k))
            first += nbx * nby
    blocks = np.concatenate(blocks)
    max_ep, max_sel = quality_to_clusters(128, blocks.shape[0])
    fe = Etc1sFrontend(hip_ctx)
    fe.init(blocks, max_ep, max_sel, 1, True)
    fe.compress()
    ept, selt = default_params(128, 1)
    be = Etc1sBackend.from_frontend(fe, slices, ept, selt, 1)
    be.encode()
    cli = run_ref_cli(tmp_path / "x.png", "-etc1s", "-q", "128", "-mipmap")
    mine = be.basis_file(key_values=basis_file_key_values(cli))
    assert mine.shape == cli.shape and (mine == cli).all()
    cli2 = run_ref_cli(tmp_path / "x.png", "-etc1s", "-q", "128", "-mipmap", ktx2=True)
    mine2 = be.ktx2_file(has_alpha=alpha, key_values=ktx2_file_key_values(cli2))
    assert mine2.shape == cli2.shape and (mine2 == cli2).all()
    be.close(); fe.close()
