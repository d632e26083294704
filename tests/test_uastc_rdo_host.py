"""CPU-only checks of the UASTC RDO post-pass (uastc_rdo, encoder/basisu_uastc_enc.cpp:3824-4163).

The GPU strips kernel and tests/native/uastc_host.cpp compile the SAME per-block pieces (basis_universal_amd/csrc/uastc_rdo.h); here the
host build, driven by a plain scalar strip loop, is held against (1) the committed known answers of the real reference
(tests/golden/uastc_rdo_vectors.npz, tools/gen_golden_uastc_rdo.py) and (2), where oracle/_ref is present, the reference itself on
fresh inputs and parameter draws. The GPU build is held to the same vectors in test_gpu_uastc_rdo.py. All comparisons are bit-exact.
"""
import ctypes as C
import pathlib

import numpy as np
import pytest

import helpers
import uastc_rdo_cases as K
from helpers import ptr

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "uastc_rdo_vectors.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,flags,jobs,kw", helpers.uastc_rdo_cases(), ids=[c[0] for c in helpers.uastc_rdo_cases()])
@pytest.mark.parametrize("table", [False, True], ids=["decode", "table"])
def test_host_rdo_matches_reference_vectors(golden, name, flags, jobs, kw, table):
    """table: trials scored from the per-block weight-error table (uastc_rdo.h, what the GPU strips kernel does) instead of decoded."""
    packed = golden[f"packed_l{flags & 7}"]
    got = helpers.host_uastc_rdo(packed, golden["blocks"], flags, jobs, table, **kw)
    bad = np.nonzero((got != golden[name]).any(1))[0]
    assert bad.size == 0, f"{name}: {bad.size} blocks differ, first {bad[:5]}"
    assert (golden[name] != packed).any(), "the case must modify something"


def test_unpack_is_the_inverse_of_pack(golden):
    """unpack_block (transcoder.cpp:15274-15735) followed by the hint recomputation and pack_block (uastc_recompute_hints, uastc_enc.cpp:
    3647-3726) must give back an encoder output bit for bit: same endpoints, weights, pattern -- and the same hints, since they are a
    function of those. Invalid mode codes must be refused like the reference does."""
    H = helpers.uastc_host()
    for level in (0, 2, 3):
        packed = golden[f"packed_l{level}"]
        again = np.ascontiguousarray(packed).copy()
        assert H.hc_rehint(ptr(np.ascontiguousarray(golden["blocks"])), packed.shape[0], level, ptr(again)) == 1
        bad = np.nonzero((again != packed).any(1))[0]
        assert bad.size == 0, f"level {level}: {bad.size} blocks change, first {bad[:5]}"
    out = np.zeros(64, np.uint8)
    junk = np.zeros(16, np.uint8)
    junk[0] = 0x45  # 7-bit prefix that is no mode code (transcoder.cpp:14376-14402)
    assert H.hc_unpack_block(ptr(junk), ptr(out)) == 0
    assert H.hc_unpack_block(ptr(np.ascontiguousarray(golden["packed_l2"][0])), ptr(out)) == 1


def test_strips_are_independent(golden):
    """uastc_rdo's total_jobs strips (uastc_enc.cpp:4103-4150) never look across their borders: strip k of a 4-job run equals a single-strip
    run over that sub-array."""
    packed, blocks = golden["packed_l2"], golden["blocks"]
    n = packed.shape[0]
    per = n // 4
    whole = helpers.host_uastc_rdo(packed, blocks, 2, 4, lam=3.0)
    for f in range(0, n, per):
        part = helpers.host_uastc_rdo(packed[f:f + per], blocks[f:f + per], 2, 0, lam=3.0)
        assert (whole[f:f + per] == part).all()


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
def test_host_rdo_vs_reference_random_params():
    rng = np.random.default_rng(5)
    img = helpers.synth(192, 128, 21)
    blocks = helpers.to_pixel_blocks(img).copy()
    blocks[700:1100, :, :, 3] = rng.integers(0, 256, size=(400, 4, 4), dtype=np.uint8)
    blocks[1100:, :, :, 3] = blocks[1100:, :, :, 1]
    # every 5th block luminance+alpha (modes 15/17, whose selector fields reach into the endpoint bits of their neighbours: the deferred
    # refit of uastc_rdo.h has to settle those first)
    grey = blocks[::5, :, :, 1].copy()
    blocks[::5, :, :, 0] = grey
    blocks[::5, :, :, 2] = grey
    blocks[::5, :, :, 3] = 255 - grey // 2
    for trial in range(7):
        if trial == 6:
            blocks = helpers.smooth_with_la_blocks(192, 128, 3)
        level = int(rng.integers(0, 3)) if trial < 6 else 0
        packed = helpers.ref_encode_uastc(blocks, level)
        kw = dict(lam=float(rng.choice([0.25, 0.75, 2.0, 6.0])), dict_size=int(rng.choice([16, 256, 4096, 16384])), refine=int(rng.integers(0, 2)),
                  skip_rms=float(rng.choice([4.0, 8.0, 20.0])), max_rms_ratio=float(rng.choice([1.1, 3.0, 10.0])),
                  smooth_scale=float(rng.choice([1.0, 10.0, 20.0])), smooth_std_dev=float(rng.choice([9.0, 18.0])), literal_cost=int(rng.choice([80, 100, 130])))
        jobs = int(rng.choice([0, 2, 4, 7]))
        if trial == 6:
            kw, jobs = dict(lam=20.0), 0
        want = helpers.ref_uastc_rdo(packed, blocks, level, jobs, **kw)
        for table in (False, True):
            got = helpers.host_uastc_rdo(packed, blocks, level, jobs, table, **kw)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, f"trial {trial} level {level} jobs {jobs} table {table} {kw}: {bad.size} blocks differ, first {bad[:5]}"


def test_counters_of_the_golden_cases_are_self_consistent(golden):
    """hc_uastc_rdo_counted: `modified` counts walks that replaced a block's selectors (a winner may carry the very bits the block had: never fewer than the blocks
    that changed), `skipped` the blocks rdo_prepare says to leave alone -- a property of the block alone, so the sum over one-block runs -- and both scoring modes
    count the same, refits included."""
    alone = {}
    for name, flags, jobs, kw in helpers.uastc_rdo_cases():
        packed, blocks = golden[f"packed_l{flags & 7}"], golden["blocks"]
        got, counts = helpers.host_uastc_rdo_counted(packed, blocks, flags, jobs, True, **kw)
        assert (got == golden[name]).all()
        if name in ("default_l2", "norefine_l0", "settle_l0"):   # the decoding form refits at once, the table form later or in front of a sensitive block: same count
            plain, plain_counts = helpers.host_uastc_rdo_counted(packed, blocks, flags, jobs, False, **kw)
            assert (plain == got).all() and plain_counts == counts, (name, counts, plain_counts)
        changed = int((got != packed).any(1).sum())
        assert counts["modified"] == changed > 0, (name, counts, changed)   # equal in these eight; in general never fewer
        assert counts["refined"] <= counts["modified"] and (counts["refined"] > 0) == bool(kw.get("refine", 1)), (name, counts)
        key = (flags & 7, kw.get("skip_rms", helpers.RDO_DEFAULTS["skip_rms"]))
        if key not in alone:
            alone[key] = sum(helpers.host_uastc_rdo_counted(packed[i:i + 1], blocks[i:i + 1], flags, 0, True, **kw)[1]["skipped"] for i in range(packed.shape[0]))
        assert counts["skipped"] == alone[key] > 0, (name, counts, alone[key])


def test_window_is_dict_size_over_sixteen_rounded_down(golden):
    """lz_dict_size 1, 15, 16 and 31 are all a window of one block, 47 is 32: pinned here so that the GPU test of such sizes has a host result that means what it
    says. 32768 on the golden blocks is the reference's own known answer (bigdict_l1, test_host_rdo_matches_reference_vectors); 32767 gives the same."""
    packed, blocks = golden["packed_l2"], golden["blocks"]
    one = helpers.host_uastc_rdo(packed, blocks, 2, 0, True, lam=3.0, dict_size=16)
    assert (one != packed).any()
    for size in (1, 15, 31):
        assert (helpers.host_uastc_rdo(packed, blocks, 2, 0, True, lam=3.0, dict_size=size) == one).all(), size
    assert (helpers.host_uastc_rdo(packed, blocks, 2, 0, True, lam=3.0, dict_size=32) != one).any()   # two blocks are not one
    assert (helpers.host_uastc_rdo(packed, blocks, 2, 0, True, lam=3.0, dict_size=47) == helpers.host_uastc_rdo(packed, blocks, 2, 0, True, lam=3.0, dict_size=32)).all()
    # 32767 -> 2047 blocks, 32768 -> 2048: equal only because the answer at this size almost never depends on the window's last block (what the period cases are for)
    assert (helpers.host_uastc_rdo(golden["packed_l1"], blocks, 1, 0, True, lam=2.0, dict_size=32767) == golden["bigdict_l1"]).all()


def test_period_cases_meet_their_condition():
    """The inputs of the window-edge tests (uastc_rdo_cases.py) on the host core alone, small periods: the windows P - 1 and P differ in at least 20 blocks, all in the
    tail, a window of 8 P gives what P gives (where the tail is one period), and with luminance-alpha tiles the strip holds sensitive modes, in the tail too."""
    for P in (5, 257):
        for la in (0, 5):
            tail = K.PERIOD_TAIL[P]
            packed, blocks = K.rdo_period_case(P, tail, K.PERIOD_SEED, la)
            (short, _), (exact, counts) = K.period_pair(P, tail, K.PERIOD_SEED, la)
            K.check_condition(P, packed, short, exact, la)
            if tail <= P:   # one period only: nothing but the twin is worth looking at
                wide = helpers.host_uastc_rdo(packed, blocks, 0, 0, True, dict_size=16 * 8 * P, **K.PERIOD_PARAMS)
                assert (wide == exact).all()
            if la:
                assert np.isin(K.modes_of(packed[P:]), K.SENSITIVE_MODES).any()


def test_inactive_case_meets_its_condition():
    packed, blocks, shared = K.inactive_case()
    n = K.INACTIVE_STRIP
    assert shared.size >= K.MIN_SHARED_FIELDS
    assert (K.modes_of(packed[n:2 * n]) == 8).all() and (K.modes_of(packed[2 * n + 1::3]) == 8).all()
    for jobs in (3, 0):
        got, counts = helpers.host_uastc_rdo_counted(packed, blocks, 0, jobs, True)
        assert (got[:2 * n] == packed[:2 * n]).all()   # a strip of skipped blocks, a strip of solid ones: nothing to do
        assert counts["skipped"] == n + (n + 2) // 3   # every noise tile and every loud one
        # a quiet block whose selectors the skipped block in front left in the history keeps them (its own cost is a match's, no candidate is strictly cheaper);
        # without that entry a candidate with the same bits would win and count as a modification
        assert (got[shared] == packed[shared]).all()
        assert 0 < counts["modified"] == int((got != packed).any(1).sum()) <= got[2 * n + 2::3].shape[0] - shared.size, counts


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("P,la,refine", [(P, la, refine) for P in K.PERIODS for la in (0, 5) for refine in (1, 0)] + [(2050, 0, 1), (2050, 5, 1)],
                         ids=lambda v: str(v))
def test_host_rdo_vs_reference_at_window_edges(P, la, refine):
    """The host core against the reference where the answer depends on the window's last block: period cases at w = P - 1 and w = P (rings of 4 / 8 and 256 / 512,
    the largest ring and the first window past it, two windows that slide through HBM), both scoring modes, bit for bit."""
    tail = K.PERIOD_TAIL[P]
    packed, blocks = K.rdo_period_case(P, tail, K.PERIOD_SEED, la)
    pair = K.period_pair(P, tail, K.PERIOD_SEED, la, refine, True)
    diff = K.check_condition(P, packed, pair[0][0], pair[1][0], la)
    print(f"P {P} la {la} refine {refine}: windows {P - 1} / {P} differ in {diff.size} of {packed.shape[0]} blocks; counts {pair[0][1]} / {pair[1][1]}")
    plain = K.period_pair(P, tail, K.PERIOD_SEED, la, refine, False)
    for k, w in enumerate((P - 1, P)):
        want = K.ref_period(P, tail, K.PERIOD_SEED, la, refine, w)
        for table, (got, counts) in ((True, pair[k]), (False, plain[k])):
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, f"P {P} w {w} table {table}: {bad.size} blocks differ, first {bad[:5]}"
        assert pair[k][1] == plain[k][1], (w, pair[k][1], plain[k][1])


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name,kw", K.PARAM_CORNERS, ids=[c[0] for c in K.PARAM_CORNERS])
def test_host_rdo_vs_reference_parameter_corners(golden, name, kw):
    packed, blocks = golden["packed_l2"][:K.CORNER_BLOCKS], golden["blocks"][:K.CORNER_BLOCKS]
    want = helpers.ref_uastc_rdo(packed, blocks, 2, 0, **kw)
    for table in (False, True):
        got, counts = helpers.host_uastc_rdo_counted(packed, blocks, 2, 0, table, **kw)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, f"{name} table {table}: {bad.size} blocks differ, first {bad[:5]}"
        print(f"{name} table {table}: {int((want != packed).any(1).sum())} blocks changed, counts {counts}")


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
def test_host_rdo_vs_reference_inactive_blocks():
    packed, blocks, _ = K.inactive_case()
    for jobs in (3, 0):
        assert (helpers.ref_uastc_rdo(packed, blocks, 0, jobs) == helpers.host_uastc_rdo(packed, blocks, 0, jobs, True)).all()


@pytest.mark.ref
@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("size", K.DICT_SIZES)
def test_host_rdo_vs_reference_odd_windows(golden, size):
    """the host expectations of the GPU test of these dictionary sizes, one strip and three"""
    packed, blocks = golden["packed_l2"], golden["blocks"]
    for jobs in (0, 3):
        assert (helpers.ref_uastc_rdo(packed, blocks, 2, jobs, lam=3.0, dict_size=size) == helpers.host_uastc_rdo(packed, blocks, 2, jobs, True, lam=3.0, dict_size=size)).all(), jobs
