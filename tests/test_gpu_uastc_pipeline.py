"""-m gpu tests of the UASTC pipeline (include/basisu_hip.h: bu_hip_uastc_pipeline_*) where it differs from the plain entry points: submissions of unlike size,
pack flags, strip count and RDO parameters that follow each other on a lane with no host synchronisation (one workspace per lane, carved two ways), ragged last
strips and the single-strip fall-back behind the finish launch that is sized without looking at the walk, a ticket's statistics, the host-side refusals, input
tiles still in flight on the caller's stream, and lanes with reserved walk CUs (bu_hip_tuning::uastc_walk_cus).

Every comparison is bit-exact against bytes that are pinned to the real encoder: the committed vectors (uastc_reference_vectors.npz, uastc_rdo_vectors.npz) where
a whole array is submitted, the host build of the same core (helpers.host_encode_uastc / host_uastc_rdo, pinned by test_uastc_core_host.py and
test_uastc_rdo_host.py) for sub-arrays -- never a second run of the pipeline. Every output region is 0xA5 before its submission runs."""
import functools
import pathlib

import numpy as np
import pytest

import helpers
from basis_universal_amd import capi, uastc
from test_gpu_uastc_rdo import params

pytestmark = pytest.mark.gpu
HERE = pathlib.Path(__file__).resolve().parent
FILL = 0xA5

RDO_A = dict(lam=1.0)
RDO_B = dict(lam=4.0, refine=0)


@functools.lru_cache(maxsize=None)
def _vectors():
    return np.load(HERE / "golden" / "uastc_rdo_vectors.npz"), np.load(HERE / "golden" / "uastc_reference_vectors.npz")


def strip_layout(n, jobs):
    """uastc_rdo's cut of n blocks into strips (uastc_enc.cpp:4103-4111) -> (blocks per strip or 0 for one strip, strips); = bu::uastc_rdo_strips, which
    test_ticket_statistics holds it to"""
    per_job = n // jobs if jobs else 0
    if jobs <= 1 or per_job <= 8:
        return 0, 1
    return per_job, -(-n // per_job)


@functools.lru_cache(maxsize=None)
def expected(source, start, n, flags, jobs, rdo):
    """The bytes of one submission: blocks [start, start + n) of `source` ("rdo": the 2,792 blocks of the RDO vectors, "enc": the 1,464 of the encoder vectors)
    at pack flags `flags`, then uastc_rdo with `jobs` strips and the parameters `rdo` (a tuple of items, None = plain encode) -> (packed, final)"""
    rv, ev = _vectors()
    blocks = (rv if source == "rdo" else ev)["blocks"]
    whole = start == 0 and n == blocks.shape[0]
    sub = np.ascontiguousarray(blocks[start:start + n])
    if whole and source == "rdo" and flags in (0, 1, 2, 3):
        packed = rv[f"packed_l{flags}"]
    elif whole and source == "enc" and flags in (0, 1, 2, 3):
        packed = ev[f"level{flags}"]
    else:
        packed = helpers.host_encode_uastc(sub, flags)
    if rdo is None:
        return packed, packed
    kw = dict(rdo)
    if whole and source == "rdo" and flags == 2 and kw == RDO_A and jobs in (0, 4):
        return packed, rv["default_l2" if jobs == 0 else "jobs4_l2"]
    return packed, helpers.host_uastc_rdo(packed, sub, flags, jobs, **kw)


class Rig:
    """The two vector files' tiles resident on one context, and a 0xA5-filled output buffer handed out region by region."""

    def __init__(self, ctx, out_blocks):
        rv, ev = _vectors()
        self.ctx = ctx
        self.n = {"rdo": rv["blocks"].shape[0], "enc": ev["blocks"].shape[0]}
        assert self.n == {"rdo": 2792, "enc": 1464}
        self.d_px = {"rdo": ctx.upload(rv["blocks"]), "enc": ctx.upload(ev["blocks"])}
        self.cap = out_blocks
        self.d_out = ctx.alloc(out_blocks * 16)
        self.reset()

    def reset(self):
        self.ctx.memset(self.d_out, FILL, self.cap * 16)
        self.ctx.sync()
        self.used = 0

    def region(self, n):
        assert self.used + n <= self.cap
        at = self.used
        self.used += n
        return at

    def px(self, source, start):
        return self.d_px[source] + start * 64

    def out(self, at):
        return self.d_out + at * 16

    def fetch(self):
        return self.ctx.download(self.d_out, (self.cap, 16), np.uint8)

    def close(self):
        for d in (*self.d_px.values(), self.d_out):
            self.ctx.free(d)


@pytest.fixture(scope="module")
def rig(hip_ctx):
    r = Rig(hip_ctx, 40960)
    yield r
    r.close()


def submit(pipe, rig, source, start, n, flags, jobs, rdo):
    at = rig.region(n)
    t = pipe.submit(rig.px(source, start), n, rig.out(at), None if rdo is None else params(**dict(rdo)), flags, jobs)
    return t, at


def differing(got, want):
    bad = np.nonzero((got != want).any(1))[0]
    return f"{bad.size} of {want.shape[0]} blocks differ, first {bad[:5]}"


# ----------------------------------------------------------------------------- 1. ragged submissions on shared lanes

A, B = tuple(sorted(RDO_A.items())), tuple(sorted(RDO_B.items()))
# (source, first block, blocks, pack flags, total_jobs, RDO parameters or None) in submission order. Ticket i + 1 runs on lane (i + 1) % lanes: the sizes go
# large large small small small small large large large large small small and the plain encodes sit at 1, 4 and 9, so that for 1, 2 and 4 lanes every lane takes a
# small submission behind a larger one and one lane runs RDO, plain encode, RDO in a row.
SUBMISSIONS = [
    ("rdo", 0, 2792, 2, 0, A),
    ("rdo", 0, 2792, 2, 0, None),
    ("rdo", 100, 257, 2, 4, B),
    ("rdo", 1500, 70, 1, 8, A),
    ("rdo", 2000, 300, 0, 0, None),
    ("rdo", 40, 35, 2, 4, B),
    ("rdo", 0, 2792, 2, 5, A),
    ("rdo", 900, 1000, 0, 3, B),
    ("rdo", 1700, 600, 2, 7, A),
    ("enc", 0, 1464, 3, 0, None),
    ("rdo", 7, 1, 2, 0, B),
    ("rdo", 2700, 64, 2, 1, A),
]
PAIRS = {(2792, 0), (2792, 5), (257, 4), (600, 7), (70, 8), (35, 4), (1, 0), (64, 1), (1000, 3)}


def modified_per_strip(s):
    """how many blocks of each strip the reference bytes of submission s change"""
    packed, want = expected(*s)
    per, strips = strip_layout(s[2], s[4])
    changed = (packed != want).any(1)
    return [int(changed[k * per:(k + 1) * per].sum()) for k in range(strips)] if per else [int(changed.sum())]


def lanes_of(lanes):
    """-> per lane, the indices into SUBMISSIONS it runs, in order (bu_hip_uastc_pipeline_submit: ticket % lanes, tickets from 1)"""
    return [[i for i in range(len(SUBMISSIONS)) if (i + 1) % lanes == lane] for lane in range(lanes)]


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_ragged_submissions_back_to_back(hip_ctx, rig, lanes):
    # what the list has to contain, checked before anything runs
    with_rdo = [s for s in SUBMISSIONS if s[5] is not None]
    assert {(s[2], s[4]) for s in with_rdo} == PAIRS
    layouts = {(s[2], s[4]): strip_layout(s[2], s[4]) for s in with_rdo}
    assert any(per and n % per for (n, _), (per, _) in layouts.items()), "no remainder strip"
    assert layouts[(2792, 5)] == (558, 6) and layouts[(600, 7)] == (85, 8) and layouts[(257, 4)] == (64, 5) and layouts[(1000, 3)] == (333, 4)
    assert layouts[(70, 8)] == (0, 1) and layouts[(35, 4)] == (0, 1), "no single-strip fall-back with total_jobs > 1"
    counts = {(s[2], s[4]): modified_per_strip(s) for s in with_rdo}
    assert counts[(600, 7)][-1] > 0 and 600 % 85, "no remainder strip with a modified block"
    # the finish launch covers every strip's list only at its full length: these strips modify more blocks than a launch for half a strip (in workgroups of 64) reaches
    assert max(counts[(2792, 5)]) > 320 > 558 // 2 and max(counts[(1000, 3)]) > 192 > 333 // 2
    per_lane = lanes_of(lanes)
    kinds = ["".join("P" if SUBMISSIONS[i][5] is None else "R" for i in idx) for idx in per_lane]
    assert any("RPR" in k for k in kinds), kinds
    for idx in per_lane:
        sizes = [SUBMISSIONS[i][2] for i in idx]
        assert any(b < a for a, b in zip(sizes, sizes[1:])), sizes   # a small submission into the workspace a larger one has just used

    rig.reset()
    pipe = uastc.UastcPipeline(hip_ctx, lanes, 2792, 3, 8)
    try:
        placed = [submit(pipe, rig, *s)[1] for s in SUBMISSIONS]
        pipe.wait(0)
    finally:
        pipe.close()
    got = rig.fetch()
    for i, (s, at) in enumerate(zip(SUBMISSIONS, placed)):
        want = expected(*s)[1]
        assert (got[at:at + s[2]] == want).all(), f"submission {i} {s}: {differing(got[at:at + s[2]], want)}"
    assert (got[rig.used:] == FILL).all()


# ----------------------------------------------------------------------------- 2. statistics

def test_ticket_statistics(hip_ctx, rig):
    """Two lanes: wait(ticket) before the lane is used again returns that submission's counters."""
    rig.reset()
    cases = [("rdo", 0, 2792, 2, 5, A), ("rdo", 0, 2792, 2, 0, None), ("rdo", 900, 1000, 0, 3, B), ("rdo", 1500, 70, 1, 8, A), ("rdo", 1800, 600, 2, 7, A), ("rdo", 100, 257, 2, 4, B)]
    pipe = uastc.UastcPipeline(hip_ctx, 2, 2792, 2, 5)   # (five strips of 558 need more workspace than eight of 349: larger histories)
    stats, placed = [], []
    try:
        for k in range(0, len(cases), 2):   # one submission per lane, then both tickets' statistics
            pair = [submit(pipe, rig, *s) for s in cases[k:k + 2]]
            placed += [at for _, at in pair]
            stats += [pipe.wait(t) for t, _ in reversed(pair)][::-1]
        pipe.wait(0)
    finally:
        pipe.close()
    got = rig.fetch()
    for s, at, st in zip(cases, placed, stats):
        packed, want = expected(*s)
        assert (got[at:at + s[2]] == want).all(), (s, differing(got[at:at + s[2]], want))
        if s[5] is None:
            assert st == {"modified": 0, "refined": 0, "skipped": 0, "strips": 0}, (s, st)
            continue
        strips = strip_layout(s[2], s[4])[1]
        changed = int((want != packed).any(1).sum())
        # (the walk's counter includes the rare block it rewrote with the bytes it already had: test_gpu_kodak24.py allows one per strip)
        assert st["strips"] == strips and 0 <= st["modified"] - changed <= strips, (s, st, changed)
        assert st["skipped"] <= s[2] and st["refined"] <= st["modified"], (s, st)
        if not dict(s[5]).get("refine", 1):
            assert st["refined"] == 0, (s, st)


# ----------------------------------------------------------------------------- 3. capacity and the other refusals

def test_refusals_are_host_side_and_leave_the_lane_usable(hip_ctx, rig):
    """A pipeline made for (1,464 blocks, level 2, 4 strips) takes exactly that and refuses what needs more workspace, whatever arena its (recycled) lane context
    came with; every refusal is decided on the host before anything is enqueued (bu_hip_uastc_pipeline_submit), and the next submission on the lane is right."""
    _, ev = _vectors()
    n = 1464
    rig.reset()
    d_px = hip_ctx.alloc(2 * n * 64)   # room for what must be refused, so that a refusal that fails to happen fails the test and nothing else
    hip_ctx.memcpy_d2d(d_px, rig.px("enc", 0), n * 64)
    hip_ctx.memcpy_d2d(d_px + n * 64, rig.px("enc", 0), n * 64)
    hip_ctx.sync()
    made_for = max(uastc.workspace_bytes(n, 2), uastc.rdo_workspace_bytes(n, 4))
    pipe = uastc.UastcPipeline(hip_ctx, 1, n, 2, 4)

    def good(rdo, jobs):
        at = rig.region(n)
        pipe.submit(d_px, n, rig.out(at), None if rdo is None else params(**dict(rdo)), 2, jobs)
        pipe.wait(0)
        got = hip_ctx.download(rig.out(at), (n, 16), np.uint8)
        want = expected("enc", 0, n, 2, jobs, rdo)[1]
        assert (got == want).all(), differing(got, want)

    def refused(d_in, blocks, d_to, rdo, flags, jobs, text):
        at = rig.region(2 * n)
        with pytest.raises(capi.HipError, match=text):
            pipe.submit(d_in, blocks, rig.out(at) if d_to else 0, rdo, flags, jobs)
        pipe.wait(0)
        hip_ctx.sync()
        assert (hip_ctx.download(rig.out(at), (2 * n, 16), np.uint8) == FILL).all(), "a refused submission wrote"
        good(None, 4)

    try:
        good(None, 4)
        assert (ev["level2"] == expected("enc", 0, n, 2, 4, None)[1]).all()
        good(A, 4)
        refused(d_px, 2 * n, True, params(**RDO_A), 2, 4, "exceed")
        assert uastc.workspace_bytes(n, 3) > made_for   # level 3 has more candidate slots per block
        refused(d_px, n, True, None, 3, 4, "exceed")
        need64 = max(uastc.workspace_bytes(n, 2), uastc.rdo_workspace_bytes(n, 64))
        if need64 > made_for:
            refused(d_px, n, True, params(**RDO_A), 2, 64, "exceed")
        else:
            good(A, 64)
        refused(d_px, 0, True, None, 2, 4, "no blocks")
        refused(0, n, True, None, 2, 4, "null pointer")
        refused(d_px, n, False, None, 2, 4, "null pointer")
        good(A, 4)
    finally:
        pipe.close()
        hip_ctx.free(d_px)


# ----------------------------------------------------------------------------- 4. refused RDO parameters

def test_refused_rdo_parameters_leave_nothing_in_flight(hip_ctx, rig):
    """lambda 0 is refused like bu_hip_k_uastc_rdo refuses it -- before the encode is enqueued: wait(0) has nothing to wait for and the output stays as it was."""
    n = 2792
    for lanes in (1, 2):
        rig.reset()
        at = rig.region(n)
        pipe = uastc.UastcPipeline(hip_ctx, lanes, n, 2, 4)
        try:
            for bad in (dict(lam=0.0), dict(max_rms_ratio=1.0), dict(dict_size=0)):
                with pytest.raises(capi.HipError, match="lambda > 0"):
                    pipe.submit(rig.px("rdo", 0), n, rig.out(at), params(**bad), 2, 4)
            pipe.wait(0)
            hip_ctx.sync()
            assert (hip_ctx.download(rig.out(at), (n, 16), np.uint8) == FILL).all(), "the refused submission's encode ran"
            # the lane is as it was
            t = pipe.submit(rig.px("rdo", 0), n, rig.out(at), params(**RDO_A), 2, 4)
            assert t == 1 and pipe.wait(t)["strips"] == 4
        finally:
            pipe.close()
        got = hip_ctx.download(rig.out(at), (n, 16), np.uint8)
        want = expected("rdo", 0, n, 2, 4, A)[1]
        assert (got == want).all(), differing(got, want)


# ----------------------------------------------------------------------------- 5. tiles still in flight on the caller's stream

def test_input_still_in_flight_on_the_callers_stream(hip_ctx, rig):
    """The tiles are produced by copies enqueued on the parent context's stream right before the submission (behind a 64 MiB fill, so that they have not run when
    submit returns): the lane's wait for the `input` event is all that orders its kernels behind them."""
    rv, _ = _vectors()
    n = 2792
    tiles = np.ascontiguousarray(rv["blocks"])
    other = np.ascontiguousarray(tiles[::-1])
    big = 64 << 20
    d_busy, d_in, d_stage = hip_ctx.alloc(big), hip_ctx.upload(other), hip_ctx.upload(tiles)
    rig.reset()
    pipe = uastc.UastcPipeline(hip_ctx, 2, n, 2, 0)
    try:
        at = rig.region(n)
        src = tiles.copy()
        hip_ctx.memset(d_busy, 1, big)
        hip_ctx.memcpy_h2d_async(d_in, src)
        pipe.submit(d_in, n, rig.out(at), params(**RDO_A), 2, 0)
        src[:] = 0   # the header's promise: the source may be released when the call returns
        pipe.wait(0)
        got = hip_ctx.download(rig.out(at), (n, 16), np.uint8)
        assert (got == rv["default_l2"]).all(), "h2d_async: " + differing(got, rv["default_l2"])

        hip_ctx.memcpy_h2d(d_in, other)   # (synchronises) the other tiles again
        at = rig.region(n)
        hip_ctx.memset(d_busy, 2, big)
        hip_ctx.memcpy_d2d(d_in, d_stage, n * 64)
        pipe.submit(d_in, n, rig.out(at), params(**RDO_A), 2, 0)
        pipe.wait(0)
        got = hip_ctx.download(rig.out(at), (n, 16), np.uint8)
        assert (got == rv["default_l2"]).all(), "d2d: " + differing(got, rv["default_l2"])
    finally:
        pipe.close()
        hip_ctx.sync()
        for d in (d_busy, d_in, d_stage):
            hip_ctx.free(d)


# ----------------------------------------------------------------------------- 6. reserved walk CUs

def test_reserved_walk_cus():
    """bu_hip_tuning::uastc_walk_cus != 0: both builds of the walk on streams masked to the reserved CUs, forked off the lane's stream and joined back
    (uastc_rdo_walks' first branch). Pipelines for 32, 0, 24 (which does not divide an MI355X's 256 CUs) and 1,024 (no device has as many: nothing to reserve) are
    made and closed in that order on one context of the test's own, so that the lanes' parked contexts have their streams re-made every time the value changes."""
    rv, _ = _vectors()
    n = 2792
    ctx = capi.Context(0)
    try:
        d_px = ctx.upload(rv["blocks"])
        d_out = ctx.alloc(4 * n * 16)
        for v in (32, 0, 24, 1024):
            ctx.set_tuning(uastc_walk_cus=v)
            assert ctx.tuning()["uastc_walk_cus"] == v
            ctx.memset(d_out, FILL, 4 * n * 16)
            pipe = uastc.UastcPipeline(ctx, 2, n, 2, 4)
            try:
                for k, jobs in enumerate((4, 0, 4, 0)):
                    pipe.submit(d_px, n, d_out + k * n * 16, params(**RDO_A), 2, jobs)
                pipe.wait(0)
            finally:
                pipe.close()
            got = ctx.download(d_out, (4, n, 16), np.uint8)
            for k, name in enumerate(("jobs4_l2", "default_l2", "jobs4_l2", "default_l2")):
                assert (got[k] == rv[name]).all(), f"walk CUs {v}, submission {k}: {differing(got[k], rv[name])}"
        ctx.free(d_px)
        ctx.free(d_out)
    finally:
        ctx.close()
