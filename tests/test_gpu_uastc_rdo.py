"""-m gpu parity tests of the UASTC RDO post-pass (include/basisu_hip.h: bu_hip_k_uastc_rdo / bu_hip_uastc_rdo).

Bit-exact against (1) the committed known answers of the real reference's uastc_rdo for every parameter case, (2) the real reference
(oracle/_ref) on a fresh image, and -- at a size the serial reference would need minutes for -- through size-independent properties:
strips are independent (strip k of a many-strip run equals a run over that sub-array alone, checked against the reference on a sample of
strips), the run is deterministic, and unmodified blocks keep every bit.
"""
import ctypes as C
import pathlib

import numpy as np
import pytest

import helpers
import uastc_rdo_cases as K
from basis_universal_amd import uastc

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "uastc_rdo_vectors.npz"
KEYS = dict(lam="m_lambda", max_rms_ratio="m_max_allowed_rms_increase_ratio", skip_rms="m_skip_block_rms_thresh", smooth_std_dev="m_max_smooth_block_std_dev",
            smooth_scale="m_smooth_block_max_error_scale", dict_size="m_lz_dict_size", literal_cost="m_lz_literal_cost", refine="m_endpoint_refinement")


def params(**kw):
    d = dict(helpers.RDO_DEFAULTS)
    d.update(kw)
    return uastc.RdoParams(**{KEYS[k]: v for k, v in d.items()})


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,flags,jobs,kw", helpers.uastc_rdo_cases(), ids=[c[0] for c in helpers.uastc_rdo_cases()])
def test_matches_reference_vectors(hip_ctx, golden, name, flags, jobs, kw):
    packed = golden[f"packed_l{flags & 7}"]
    got, info = uastc.uastc_rdo(hip_ctx, packed, golden["blocks"], params(**kw), flags, jobs)
    want = golden[name]
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"{name}: {bad.size} blocks differ, first {bad[:5]}: got {got[bad[:1]].tobytes().hex()} want {want[bad[:1]].tobytes().hex()}"
    _, counts = helpers.host_uastc_rdo_counted(packed, golden["blocks"], flags, jobs, True, **kw)
    assert {k: info[k] for k in counts} == counts
    assert info["modified"] == int((want != packed).any(1).sum())   # in general ">=": a winner may carry the bits the block had; equal in all eight cases


def test_flagged_and_unflagged_strips_side_by_side(hip_ctx, golden):
    """The walk comes in two builds: strips that hold a block of a sensitive mode (15 / 17 / 18: the prepare pass flags them) take the one with the colour-cell
    refit in it, all others the lean one (no refit, four waves per SIMD), both launched over all strips on two streams. Pure RGB blocks in front of the vectors'
    alpha classes give batches in which some strips are flagged and some are not, for several strip counts; with endpoint refinement off nothing is flagged.
    Same bytes as the host build of the same core (pinned to the reference by tests/test_uastc_rdo_host.py) every time."""
    packed, blocks = golden["packed_l2"], golden["blocks"]
    modes = np.array(helpers.UASTC_HUFF_MODES)[packed[:, 0] & 127]
    plain = np.nonzero(~np.isin(modes, (8, 15, 16, 17)))[0]
    order = np.concatenate([plain, np.setdiff1d(np.arange(packed.shape[0]), plain)])   # opaque modes first, the alpha / luminance-alpha classes last
    pk, bl = np.ascontiguousarray(packed[order]), np.ascontiguousarray(blocks[order])
    for jobs in (0, 2, 4, 7):
        for refine in (1, 0):
            got, _ = uastc.uastc_rdo(hip_ctx, pk, bl, params(lam=3.0, refine=refine), 2, jobs)
            assert (got == helpers.host_uastc_rdo(pk, bl, 2, jobs, lam=3.0, refine=refine)).all(), (jobs, refine)


@pytest.mark.parametrize("n", [0, 1, 2, 35, 36, 37, 40, 257, 600])
@pytest.mark.parametrize("jobs", [0, 4])
def test_ragged_sizes(hip_ctx, golden, n, jobs):
    """35, 36, 37 at four jobs: one strip (per_job 8), the smallest size that is split (four strips of 9), a fifth strip of one block"""
    packed, blocks = golden["packed_l2"][:n], golden["blocks"][:n]
    got, info = uastc.uastc_rdo(hip_ctx, packed, blocks, params(lam=4.0), 2, jobs)
    assert got.shape == (n, 16)
    assert (got == helpers.host_uastc_rdo(packed, blocks, 2, jobs, lam=4.0)).all()
    if n in (35, 36, 37):
        assert info["strips"] == ({35: 1, 36: 4, 37: 5}[n] if jobs == 4 else 1)


def test_window_larger_than_the_lds_ring(hip_ctx, golden):
    """lz_dict_size 65536 -> a look-back of 4096 blocks: past the 2048-block LDS ring, the strips kernel reads its candidates back from HBM
    (k_rdo_strips<false>); same bytes as the host build of the same core, and as the ring version where the window never fills."""
    packed, blocks = golden["packed_l2"], golden["blocks"]
    got, _ = uastc.uastc_rdo(hip_ctx, packed, blocks, params(lam=3.0, dict_size=65536), 2, 0)
    assert (got == helpers.host_uastc_rdo(packed, blocks, 2, 0, lam=3.0, dict_size=65536)).all()
    small, _ = uastc.uastc_rdo(hip_ctx, packed[:1500], blocks[:1500], params(lam=3.0, dict_size=65536), 2, 0)
    ring, _ = uastc.uastc_rdo(hip_ctx, packed[:1500], blocks[:1500], params(lam=3.0, dict_size=32768), 2, 0)
    assert (small == ring).all()   # 1500 blocks: both windows reach back to the strip's first block


def test_blocking_host_pointer_entry(hip_ctx, golden):
    blocks = np.ascontiguousarray(golden["blocks"])
    n = blocks.shape[0]
    hip_ctx.check(hip_ctx.lib.set_pixel_blocks(hip_ctx.h, n, blocks.ctypes.data), "set_pixel_blocks")
    out = np.ascontiguousarray(golden["packed_l2"]).copy()
    p = uastc.RdoParams()
    hip_ctx.lib.uastc_rdo_default_params(C.byref(p))
    assert (p.m_lambda, p.m_lz_dict_size, p.m_endpoint_refinement) == (0.5, 4096, 1)
    p.m_lambda = 1.0
    stats = (C.c_uint32 * 4)()
    hip_ctx.check(hip_ctx.lib.uastc_rdo(hip_ctx.h, out.ctypes.data, C.byref(p), 2, 0, stats), "uastc_rdo")
    assert (out == golden["default_l2"]).all()
    assert stats[0] == int((golden["default_l2"] != golden["packed_l2"]).any(1).sum()) and stats[3] == 1


def test_rejects_bad_arguments(hip_ctx, golden):
    packed, blocks = golden["packed_l2"][:64], golden["blocks"][:64]
    with pytest.raises(Exception):
        uastc.uastc_rdo(hip_ctx, packed, blocks, params(lam=0.0), 2, 0)
    with pytest.raises(Exception):
        uastc.uastc_rdo(hip_ctx, packed, blocks, params(max_rms_ratio=1.0), 2, 0)
    junk = packed.copy()
    junk[5, 0] = 0x45  # not a mode code: the reference's unpack fails and uastc_rdo returns false
    with pytest.raises(Exception):
        uastc.uastc_rdo(hip_ctx, junk, blocks, params(), 2, 0)


@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
def test_vs_reference_fresh_image(hip_ctx):
    rng = np.random.default_rng(9)
    blocks = helpers.to_pixel_blocks(helpers.synth(512, 256, 33)).copy()
    blocks[3000:5000, :, :, 3] = blocks[3000:5000, :, :, 2] // 2 + 100
    for level, jobs, kw in [(2, 4, dict(lam=1.0)), (1, 0, dict(lam=3.0, dict_size=8192)), (0, 16, dict(lam=5.0, refine=0))]:
        packed = uastc.encode_uastc_blocks(hip_ctx, blocks, level)
        want = helpers.ref_uastc_rdo(packed, blocks, level, jobs, **kw)
        got, info = uastc.uastc_rdo(hip_ctx, packed, blocks, params(**kw), level, jobs)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, f"level {level} jobs {jobs} {kw}: {bad.size} of {blocks.shape[0]} blocks differ, first {bad[:5]}"
        assert info["modified"] == int((want != packed).any(1).sum())


def test_large_image_properties(hip_ctx):
    """2048x2048 (262,144 blocks), 64 strips, everything device-resident: deterministic; each strip equals a run over that strip alone
    (two sampled strips, also against the CPU reference when present); unmodified blocks are bit-identical to the input."""
    blocks = helpers.to_pixel_blocks(helpers.synth(2048, 2048, 77))
    n = blocks.shape[0]
    d_px = hip_ctx.upload(blocks)
    d_blk = hip_ctx.alloc(n * 16)
    try:
        uastc.encode_uastc_blocks(hip_ctx, d_px, 2, n_blocks=n, out_device=d_blk)
        packed = hip_ctx.download(d_blk, (n, 16), np.uint8)
        _, info = uastc.uastc_rdo(hip_ctx, d_blk, d_px, params(lam=2.0), 2, 64, n_blocks=n)
        got = hip_ctx.download(d_blk, (n, 16), np.uint8)
        assert info["strips"] == 64 and info["modified"] == int((got != packed).any(1).sum())
        again, _ = uastc.uastc_rdo(hip_ctx, packed, blocks, params(lam=2.0), 2, 64)
        assert (again == got).all()
        per = n // 64
        for k in (0, 37):
            sl = slice(k * per, (k + 1) * per)
            alone, _ = uastc.uastc_rdo(hip_ctx, packed[sl], blocks[sl], params(lam=2.0), 2, 0)
            assert (alone == got[sl]).all()
            if helpers.have_ref():
                assert (helpers.ref_uastc_rdo(packed[sl], blocks[sl], 2, 0, lam=2.0) == got[sl]).all()
    finally:
        hip_ctx.free(d_px)
        hip_ctx.free(d_blk)


# ---- where the look-back window slides and ends, windows that are not the ring's size, inactive blocks, parameter corners (inputs: uastc_rdo_cases.py)

def strips_of(n, jobs):
    per_job = n // jobs if jobs else 0   # uastc_rdo, uastc_enc.cpp:4103-4111
    return 1 if jobs <= 1 or per_job <= 8 else -(-n // per_job)


def check_device(ctx, packed, blocks, flags, jobs, want=None, ref=None, **kw):
    """One device run held bit for bit to the host build of the same core (want = (bytes, counts) where the caller has them already) and, where it is built, to the
    reference; the three counters and the strip count to the counted host entry. Returns the device's bytes."""
    want, counts = want if want is not None else helpers.host_uastc_rdo_counted(packed, blocks, flags, jobs, True, **kw)
    got, info = uastc.uastc_rdo(ctx, packed, blocks, params(**kw), flags, jobs)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"jobs {jobs} {kw}: {bad.size} of {got.shape[0]} blocks differ from the host core, first {bad[:5]}: got {got[bad[:1]].tobytes().hex()} want {want[bad[:1]].tobytes().hex()}"
    assert info == dict(counts, strips=strips_of(got.shape[0], jobs)), f"jobs {jobs} {kw}"
    if helpers.have_ref():
        ref = ref if ref is not None else helpers.ref_uastc_rdo(packed, blocks, flags, jobs, **kw)
        bad = np.nonzero((got != ref).any(1))[0]
        assert bad.size == 0, f"jobs {jobs} {kw}: {bad.size} blocks differ from the reference, first {bad[:5]}"
    return got


def period_expectations(P, la, w_index):
    """The host pair of a period case with its condition checked, and the reference at that window where it is built."""
    tail = K.PERIOD_TAIL[P]
    packed, blocks = K.rdo_period_case(P, tail, K.PERIOD_SEED, la)
    pair = K.period_pair(P, tail, K.PERIOD_SEED, la)
    K.check_condition(P, packed, pair[0][0], pair[1][0], la)
    ref = K.ref_period(P, tail, K.PERIOD_SEED, la, 1, P - 1 + w_index) if helpers.have_ref() else None
    return packed, blocks, pair[w_index], ref


@pytest.mark.parametrize("edge", [0, 1], ids=["short", "exact"])
@pytest.mark.parametrize("la", [0, 5], ids=["rgb", "la5"])
@pytest.mark.parametrize("P", K.PERIODS_PAST_THE_RING)
def test_window_edge(hip_ctx, P, la, edge):
    """Block i - window is a candidate and block i - window - 1 is not. The twin of every tail block of a period case lies exactly P blocks back and is all but the
    only candidate the tight ratio admits, so the windows P - 1 ("short") and P ("exact") give different bytes (condition, checked on the host first: at least 20
    blocks, all in the tail). P = 5: rings of 4 and 8; 257: rings of 256 and 512; 2049: the largest ring, then the build that reads its candidates back from HBM;
    2050: that build at its two smallest windows (a look-back one block too long at the handover shows here, not at 2049, where the block past the window is no
    twin); 4097: that build with a window that slides. With every 5th tile luminance + alpha the strip takes the build with the refit in it, and settles windows
    that have slid. The window under test is held to the host core, the reference and the counters; the other one is run on the device only, to name the blocks in
    which the two device results differ."""
    packed, blocks, want, ref = period_expectations(P, la, edge)
    got = check_device(hip_ctx, packed, blocks, 0, 0, want, ref, dict_size=16 * (P - 1 + edge), **K.PERIOD_PARAMS)
    other, _ = uastc.uastc_rdo(hip_ctx, packed, blocks, params(dict_size=16 * (P - edge), **K.PERIOD_PARAMS), 0, 0)
    diff = np.nonzero((got != other).any(1))[0]
    assert diff.size >= K.MIN_DIFFERING and diff.min() >= P, f"windows {P - 1} and {P} on the device differ in {diff.size} blocks, first {diff[:5]}"


def test_two_hbm_strips_side_by_side(hip_ctx):
    """Two strips of 4400 blocks, a look-back of 4096: the lean HBM build walks strip 0 and the HBM build with the refit in it strip 1 (luminance-alpha tiles only
    there), each on its stream, both windows sliding. Each strip is a period case of P = 4097 on its own: its twin lies one block outside the window."""
    P, tail = 4097, K.PERIOD_TAIL[4097]
    assert 2 * (P + tail) == 2 * 4400
    parts = [period_expectations(P, la, 0) for la in (0, 5)]
    packed, blocks = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in (0, 1))
    assert not np.isin(K.modes_of(parts[0][0]), K.SENSITIVE_MODES).any()   # strip 0 goes to the lean build
    want = np.concatenate([p[2][0] for p in parts]), {k: parts[0][2][1][k] + parts[1][2][1][k] for k in parts[0][2][1]}   # strips are independent, counters add up
    ref = np.concatenate([p[3] for p in parts]) if helpers.have_ref() else None
    check_device(hip_ctx, packed, blocks, 0, 2, want, ref, dict_size=65536, **K.PERIOD_PARAMS)


@pytest.mark.parametrize("jobs", [0, 3])
@pytest.mark.parametrize("dict_size", K.DICT_SIZES)
def test_windows_that_are_not_the_rings_size(hip_ctx, golden, dict_size, jobs):
    """Windows of 1 (dictionaries below 32 bytes), 2, 3 in a ring of 4, 187 in 256, 1250 and 2047 in 2048, and 2048 out of a dictionary that is no multiple of 16."""
    check_device(hip_ctx, golden["packed_l2"], golden["blocks"], 2, jobs, lam=3.0, dict_size=dict_size)


@pytest.mark.parametrize("jobs", [3, 0])
def test_inactive_blocks(hip_ctx, jobs):
    """A strip in which every block is skipped, one of solid blocks only, one that interleaves skipped, solid and active blocks (uastc_rdo_cases.inactive_case); as
    three strips and as one. A skipped block is thread 0's alone: it enters the ring and the history, and there decides what the selectors of a later block cost."""
    packed, blocks, shared = K.inactive_case()
    n = K.INACTIVE_STRIP
    assert shared.size >= K.MIN_SHARED_FIELDS
    want = helpers.host_uastc_rdo_counted(packed, blocks, 0, jobs, True)
    assert want[1]["skipped"] >= n and want[1]["modified"] == int((want[0] != packed).any(1).sum()) > 0
    got = check_device(hip_ctx, packed, blocks, 0, jobs, want)
    assert (got[:2 * n] == packed[:2 * n]).all()   # the skipped strip and the solid strip come back as they went
    assert (got[shared] == packed[shared]).all()


@pytest.mark.parametrize("name,kw", K.PARAM_CORNERS, ids=[c[0] for c in K.PARAM_CORNERS])
def test_parameter_corners(hip_ctx, golden, name, kw):
    check_device(hip_ctx, golden["packed_l2"][:K.CORNER_BLOCKS], golden["blocks"][:K.CORNER_BLOCKS], 2, 0, **kw)
