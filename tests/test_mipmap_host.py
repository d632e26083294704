"""Mip generation, the host half on the CPU: the resampling plan bu_mipmap_plan builds (contributor lists of both axes,
pass order, sRGB tables = what Resampler / image_resample decide before touching pixels) is applied here by a float32 numpy emulation of
mipmap_kernels.hip -- same operations, same order -- and the result has to equal the REAL image_resample (oracle/_ref) byte for byte.
The GPU test (tests/test_gpu_mipmap.py) then only has to show that the kernels do what the emulation does."""
import functools
import pathlib

import numpy as np
import pytest

from helpers import have_ref, ref, synth, uniform_random
import native_libs

needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref not present")
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "resample_vectors.npz"   # tools/gen_golden_resample.py
SEEDS = ((1, False), (2, True))   # (seed, noise) of rgba(): a smooth image and uniform noise


def plan(sw, sh, dw, dh, srgb, flt, scale, wrap):
    from basis_universal_amd.etc1s import load_frontend_library
    L = load_frontend_library()
    f = L.bu_mipmap_plan
    counts = np.zeros(4, np.uint32)
    assert f(sw, sh, dw, dh, int(srgb), flt.encode(), scale, int(wrap), counts.ctypes.data, *([None] * 8))
    xf, xp, xw = np.zeros(dw + 1, np.uint32), np.zeros(counts[0], np.uint16), np.zeros(counts[0], np.float32)
    yf, yp, yw = np.zeros(dh + 1, np.uint32), np.zeros(counts[1], np.uint16), np.zeros(counts[1], np.float32)
    t0, t1 = np.zeros(256, np.float32), np.zeros(8192, np.uint8)
    assert f(sw, sh, dw, dh, int(srgb), flt.encode(), scale, int(wrap), counts.ctypes.data, *[a.ctypes.data for a in (xf, xp, xw, yf, yp, yw, t0, t1)])
    return dict(x=(xf, xp, xw), y=(yf, yp, yw), x_after_y=bool(counts[2]), identity=bool(counts[3]), to_linear=t0, to_srgb=t1)


def plan_refused(sw, sh, dw, dh, srgb, flt, scale, wrap):
    """-> the text bu_mipmap_plan leaves when it returns 0; asserts that it does"""
    from basis_universal_amd import capi
    from basis_universal_amd.etc1s import load_frontend_library
    counts = np.zeros(4, np.uint32)
    assert load_frontend_library().bu_mipmap_plan(sw, sh, dw, dh, int(srgb), flt.encode(), scale, int(wrap), counts.ctypes.data, *([None] * 8)) == 0
    return capi.load_library().last_error(None)


def emulate(src, dw, dh, p, srgb, num_comps, other_order=False, zero_start_swapped=False, reversed_taps=False):
    """mipmap_kernels.hip in numpy float32, and what bu_generate_mipmap_level does instead of launching them for an identity plan. The three flags break it on
    purpose (test_fixture_tells_wrong_from_right): the pass order the plan did not pick, the other pass starting its sum from zero, every list summed backwards."""
    if p["identity"]:
        return src.copy()
    sh, sw = src.shape[:2]
    lin = np.empty((sh, sw, 4), np.float32)
    lin[..., :3] = p["to_linear"][src[..., :3]]
    lin[..., 3] = src[..., 3].astype(np.float32) * np.float32(1.0 / 255.0)

    def along(axis_taps, data, n_out, axis, start_from_zero):
        first, pixel, weight = axis_taps
        shape = list(data.shape); shape[axis] = n_out
        out = np.zeros(shape, np.float32)
        for i in range(n_out):
            acc = None
            for k in list(range(first[i], first[i + 1]))[::-1 if reversed_taps else 1]:
                term = (data[:, pixel[k]] if axis == 1 else data[pixel[k]]) * weight[k]
                acc = (np.zeros_like(term) + term if start_from_zero else term) if acc is None else acc + term
            if axis == 1:
                out[:, i] = acc
            else:
                out[i] = acc
        return out
    x_zero, y_zero = (False, True) if zero_start_swapped else (True, False)
    if p["x_after_y"] == other_order:
        res = along(p["y"], along(p["x"], lin, dw, 1, x_zero), dh, 0, y_zero)
    else:
        res = along(p["x"], along(p["y"], lin, dh, 0, y_zero), dw, 1, x_zero)
    res = np.clip(res, np.float32(0), np.float32(1))
    out = np.zeros((dh, dw, 4), np.uint8)
    out[..., 3] = 255
    for c in range(num_comps):
        if srgb and c < 3:
            j = (np.float32(8191.0) * res[..., c] + np.float32(.5)).astype(np.int32)
            out[..., c] = p["to_srgb"][np.clip(j, 0, 8191)]
        else:
            j = (np.float32(255.0) * res[..., c] + np.float32(.5)).astype(np.int32)
            out[..., c] = np.clip(j, 0, 255)
    return out


def reference(src, dw, dh, srgb, flt, scale, wrap, num_comps):
    R = ref()
    src = np.ascontiguousarray(src)
    out = np.zeros((dh, dw, 4), np.uint8)
    assert R.ref_image_resample(src.ctypes.data, src.shape[1], src.shape[0], out.ctypes.data, dw, dh, int(srgb), flt.encode(), scale, int(wrap), 0, num_comps)
    return out


def rgba(w, h, seed, noise=False):
    img = uniform_random(w, h, seed) if noise else synth((w + 3) // 4 * 4, (h + 3) // 4 * 4, seed)[:h, :w].copy()
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 3] = np.clip(128 + 120 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img)


CASES = [  # src w, h, dst w, h, srgb, filter, scale, wrap, comps
    (64, 48, 32, 24, True, "kaiser", 1.0, True, 3),       # the compressor's defaults
    (64, 48, 32, 24, True, "kaiser", 1.0, True, 4),
    (64, 48, 32, 24, False, "kaiser", 1.0, False, 4),
    (33, 19, 16, 9, True, "kaiser", 1.0, True, 4),        # odd sizes
    (7, 5, 3, 2, True, "kaiser", 1.0, True, 3),
    (2, 2, 1, 1, True, "kaiser", 1.0, True, 4),
    (3, 1, 1, 1, True, "kaiser", 1.0, False, 4),          # one axis already at 1: magnification branch of make_clist
    (1, 4, 1, 2, True, "kaiser", 1.0, True, 3),
    (96, 16, 48, 8, True, "box", 1.0, True, 4),
    (96, 16, 48, 8, True, "tent", 1.0, False, 3),
    (40, 40, 20, 20, True, "lanczos4", 1.0, True, 4),
    (40, 40, 20, 20, False, "mitchell", 1.0, False, 3),
    (40, 40, 20, 20, True, "blackman", 1.0, True, 3),
    (40, 40, 20, 20, True, "lanczos12", 1.0, True, 3),
    (40, 40, 20, 20, True, "bell", 1.0, True, 3),
    (40, 40, 20, 20, True, "catmullrom", 1.0, False, 4),
    (48, 32, 24, 16, True, "kaiser", 1.5, True, 3),       # -mip_scale
    (48, 32, 24, 16, True, "kaiser", 0.75, False, 4),
    (160, 8, 80, 4, True, "kaiser", 1.0, True, 4),        # very different axis costs: the other pass order
    (8, 160, 4, 80, True, "kaiser", 1.0, True, 4),
    (16, 64, 16, 32, True, "kaiser", 1.0, True, 4),       # only y shrinks: x is resampled after y (Resampler's delayed x pass)
    (24, 96, 20, 32, False, "lanczos3", 1.0, False, 3),
]


# What -resample (box, clamp, 4 components: source.resample_resident), -resample_factor above 1 and -mip_slow reach beyond CASES, each at the smallest shape that
# still reaches it, with the pass order the plan has to pick: the y-first kernels (k_first_y, k_second<false>) with more than one 256-wide workgroup along x,
# magnification, one axis growing while the other shrinks, lists of thousands of taps, and image_resample's shortcut for equal sizes at scale 1.
X_FIRST, Y_FIRST, IDENTITY = "x first", "y first", "identity"
_WIDE_AND_MAGNIFY = [  # (src w, h, dst w, h, srgb, filter, scale, wrap, comps), pass order
    ((260, 6, 520, 9, True, "box", 1.0, False, 4), Y_FIRST),          # -resample upwards: k_first_y with 2 workgroups along x, k_second<false> with 3
    ((260, 6, 520, 9, True, "kaiser", 1.0, True, 4), Y_FIRST),        # ... with 6-tap lists and wrapped indices
    ((257, 5, 513, 5, True, "box", 1.0, False, 4), Y_FIRST),          # one lane into the second and into the third workgroup; height unchanged
    ((300, 5, 300, 2, True, "kaiser", 1.0, True, 4), Y_FIRST),        # only y shrinks, on a wide row
    ((6, 260, 9, 520, True, "kaiser", 1.0, True, 3), X_FIRST),        # the transposed case
    ((5, 300, 2, 300, False, "kaiser", 1.0, False, 4), X_FIRST),      # only x shrinks, on a tall image; linear
    ((520, 4, 260, 9, True, "kaiser", 1.0, True, 3), X_FIRST),        # x shrinks while y grows
    ((21, 13, 30, 9, True, "box", 1.0, False, 4), Y_FIRST),           # x grows while y shrinks: -resample 30 9
    ((21, 13, 40, 30, True, "box", 1.0, False, 4), Y_FIRST),          # magnification, every list shape: -resample 40 30
    ((7, 5, 20, 11, True, "kaiser", 1.0, True, 4), Y_FIRST),
    ((7, 5, 20, 11, True, "lanczos4", 1.0, False, 3), Y_FIRST),
    ((1, 1, 5, 3, True, "box", 1.0, False, 4), Y_FIRST),              # a 1x1 source
    ((3, 2, 300, 2, True, "tent", 1.0, True, 4), Y_FIRST),
    ((512, 3, 1, 1, True, "kaiser", 1.0, True, 4), X_FIRST),          # long lists, the -mip_slow shape: 3072 taps along x
    ((256, 4, 1, 1, True, "kaiser", 1.0, True, 3), X_FIRST),
    ((64, 64, 1, 1, True, "lanczos12", 1.0, True, 3), X_FIRST),
    ((10, 10, 10, 10, True, "kaiser", 1.5, True, 4), X_FIRST),        # equal size with scale != 1: NOT the shortcut
    ((20, 28, 20, 28, True, "box", 1.0, False, 4), IDENTITY),         # the shortcut: dst = src
    ((16, 16, 16, 16, True, "kaiser", 1.0, True, 3), IDENTITY),       # ... all four channels, although only three are asked for
]
WIDE_AND_MAGNIFY = [case for case, _ in _WIDE_AND_MAGNIFY]
PASS_ORDER = dict(_WIDE_AND_MAGNIFY)
# Further noise seeds, searched for (seeds 1..40) on the float32 emulation alone: with these inputs a byte moves when the passes run in the order the plan did not pick
# or when a list is summed backwards. With SEEDS alone the first of the two changes no byte of any case (a few ulps of a float sum move about one byte in 10^5).
EXTRA_SEEDS = {
    (260, 6, 520, 9, True, "kaiser", 1.0, True, 4): ((3, True),),
    (6, 260, 9, 520, True, "kaiser", 1.0, True, 3): ((37, True),),
    (520, 4, 260, 9, True, "kaiser", 1.0, True, 3): ((20, True),),
    (7, 5, 20, 11, True, "kaiser", 1.0, True, 4): ((26, True),),
    (5, 300, 2, 300, False, "kaiser", 1.0, False, 4): ((4, True),),
    (7, 5, 20, 11, True, "lanczos4", 1.0, False, 3): ((35, True),),
}
REFUSED = (40, 24, 20, 12, True, "box", 0.4, False, 4)   # a box of 0.4 source samples between destination centres 2 apart: some destination sample has no contributor


def case_id(case):
    return "-".join(str(v) for v in case)


def seeds_of(case):
    return SEEDS + EXTRA_SEEDS.get(case, ())


def pass_order(p):
    return IDENTITY if p["identity"] else (Y_FIRST if p["x_after_y"] else X_FIRST)


def emulated(case, seed, noise, **breaks):
    """-> (the plan's pass order, the float32 emulation's bytes) for rgba(w, h, seed, noise)"""
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
    p = plan(sw, sh, dw, dh, srgb, flt, scale, wrap)
    return pass_order(p), emulate(rgba(sw, sh, seed, noise), dw, dh, p, srgb, comps, **breaks)


@functools.lru_cache(maxsize=None)
def golden():
    """-> {(case, seed): the reference's bytes}, read-only and shared, after checking that the fixture's case table is WIDE_AND_MAGNIFY"""
    arrays, meta = native_libs.load_npz_golden(GOLDEN)
    assert [tuple(c) for c in meta["cases"]] == WIDE_AND_MAGNIFY and set(EXTRA_SEEDS) <= set(WIDE_AND_MAGNIFY), "rerun tools/gen_golden_resample.py"
    assert [[tuple(s) for s in seeds] for seeds in meta["seeds"]] == [list(seeds_of(c)) for c in WIDE_AND_MAGNIFY], "rerun tools/gen_golden_resample.py"
    assert meta["pass_order"] == [PASS_ORDER[c] for c in WIDE_AND_MAGNIFY]
    return {(case, seed): arrays[f"out{k}_seed{seed}"] for k, case in enumerate(WIDE_AND_MAGNIFY) for seed, _ in seeds_of(case)}


@needs_ref
@pytest.mark.parametrize("case", CASES + WIDE_AND_MAGNIFY, ids=case_id)
def test_plan_applied_in_float32_matches_image_resample(case):
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
    for seed, noise in seeds_of(case):
        order, got = emulated(case, seed, noise)
        assert case not in PASS_ORDER or order == PASS_ORDER[case], (order, PASS_ORDER[case])
        exp = reference(rgba(sw, sh, seed, noise), dw, dh, srgb, flt, scale, wrap, comps)
        assert (got == exp).all(), (np.argwhere(got != exp)[:5], got[got != exp][:5], exp[got != exp][:5])


def test_both_pass_orders_occur():
    orders = {plan(sw, sh, dw, dh, True, "kaiser", 1.0, True)["x_after_y"] for sw, sh, dw, dh in [(16, 64, 16, 32), (1, 4, 1, 2), (64, 48, 32, 24)]}
    assert orders == {True, False}
    # ... and each case of the second list takes the order it was chosen for: a plan change that flips one fails here instead of silently losing the coverage
    got = {case: pass_order(plan(*case[:8])) for case in WIDE_AND_MAGNIFY}
    assert got == PASS_ORDER, {case_id(c): (got[c], PASS_ORDER[c]) for c in WIDE_AND_MAGNIFY if got[c] != PASS_ORDER[c]}
    assert {X_FIRST, Y_FIRST, IDENTITY} == set(got.values())
    wide = [c for c in WIDE_AND_MAGNIFY if PASS_ORDER[c] == Y_FIRST and c[0] > 256 and c[2] > 512]
    assert wide, "no y-first case with two workgroups along x in the first pass and three in the second"


@pytest.mark.parametrize("case", WIDE_AND_MAGNIFY, ids=case_id)
def test_fixture_equals_the_float32_emulation(case):
    """tests/golden/resample_vectors.npz holds what ref_image_resample wrote; needs no oracle/_ref, so it pins the emulation -- and through tests/test_gpu_mipmap.py
    the kernels -- wherever the suite runs"""
    for seed, noise in seeds_of(case):
        order, got = emulated(case, seed, noise)
        exp = golden()[case, seed]
        assert order == PASS_ORDER[case]
        assert got.shape == exp.shape and (got == exp).all(), (seed, np.argwhere(got != exp)[:5])


@needs_ref
@pytest.mark.parametrize("case", WIDE_AND_MAGNIFY, ids=case_id)
def test_fixture_equals_image_resample(case):
    sw, sh, dw, dh, srgb, flt, scale, wrap, comps = case
    for seed, noise in seeds_of(case):
        exp = reference(rgba(sw, sh, seed, noise), dw, dh, srgb, flt, scale, wrap, comps)
        assert (golden()[case, seed] == exp).all(), seed


def test_fixture_tells_wrong_from_right():
    """The emulation broken on purpose has to leave the fixture: the pass order the plan did not pick (intermediate sums round differently), and every list summed
    backwards. Which pass starts its sum from zero is NOT observable in bytes: 0.0f + t is t for every float but -0.0f, and -0.0f and +0.0f quantise to the same
    byte (see docs/HISTORY.md); that break is run to show that it changes nothing."""
    changed = {"other_order": 0, "reversed_taps": 0, "zero_start_swapped": 0}
    for case in WIDE_AND_MAGNIFY:
        if PASS_ORDER[case] == IDENTITY:
            continue
        for how in changed:
            changed[how] += any((emulated(case, seed, noise, **{how: True})[1] != golden()[case, seed]).any() for seed, noise in seeds_of(case))
    print("cases changed by each break:", changed)
    assert changed["other_order"] > 0 and changed["reversed_taps"] > 0 and changed["zero_start_swapped"] == 0, changed


def test_a_filter_scale_that_starves_a_sample_is_refused():
    """Resampler::make_clist gives up on the same sample. The reference itself is NOT run on this case: its Resampler constructor returns early with a status that
    image_resample never reads, and put_line then works on members nobody initialised -- it returned false in some runs here and crashed the process in others."""
    assert "without contributors" in plan_refused(*REFUSED[:8])


@pytest.mark.parametrize("args,reason", [
    ((40, 24, 20, 12, True, "gauss", 1.0, False), 'unknown filter "gauss"'),
    ((16385, 4, 8, 2, True, "box", 1.0, False), "source size 16385x4 is outside 1..16384"),
    ((8, 0, 8, 2, True, "box", 1.0, False), "source size 8x0 is outside 1..16384"),
    ((8, 2, 16385, 2, True, "box", 1.0, False), "destination size 16385x2 is outside 1..16384"),   # image_resample refuses the destination as well
    ((8, 2, 4, 16385, True, "kaiser", 1.0, True), "destination size 4x16385 is outside 1..16384"),
    ((8, 2, 0, 2, True, "box", 1.0, False), "destination size 0x2 is outside 1..16384"),
    (REFUSED[:8], "leaves a destination sample without contributors along x (40 -> 20)"),
])
def test_a_refused_plan_names_the_call_and_the_reason(args, reason):
    """both entry points leave "<call>: <reason>" where ctx.check reads it (without a context: the global text), not whatever an earlier call left there"""
    from basis_universal_amd import capi
    from basis_universal_amd.etc1s import load_frontend_library
    hip, L = capi.load_library(), load_frontend_library()
    hip.dll.bu_hip_set_last_error(None, b"stale")
    text = plan_refused(*args)
    assert text.startswith("bu_mipmap_plan: ") and reason in text, text
    sw, sh, dw, dh, srgb, flt, scale, wrap = args
    hip.dll.bu_hip_set_last_error(None, b"stale")
    assert L.bu_generate_mipmap_level(None, None, sw, sh, None, dw, dh, int(srgb), flt.encode(), scale, int(wrap), 4) == 0   # refused before the context is looked at
    text = hip.last_error(None)
    assert text.startswith("bu_generate_mipmap_level: ") and reason in text, text
    assert L.bu_host_last_exception().decode() == text


def test_mip_chain_sizes():
    from basis_universal_amd.etc1s import load_frontend_library
    L = load_frontend_library()
    out = np.zeros(64, np.uint32)
    n = L.bu_mipmap_level_sizes(130, 67, 1, out.ctypes.data, 32)
    assert out[:2 * n].reshape(-1, 2).tolist() == [[65, 33], [32, 16], [16, 8], [8, 4], [4, 2], [2, 1], [1, 1]]
    assert L.bu_mipmap_level_sizes(1, 1, 1, out.ctypes.data, 32) == 0
    assert L.bu_mipmap_level_sizes(256, 256, 16, out.ctypes.data, 32) == 4
