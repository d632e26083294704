"""-m gpu tests of the context's copy / stream / lifetime entry points of include/basisu_hip.h that nothing else names: bu_hip_memcpy_h2d_async (the pinned staging
ring: 4 MiB pieces, 256-byte slots, recycled when it wraps), bu_hip_memcpy_d2d, bu_hip_memcpy_d2h with and without a wait hook (the pinned bounce buffer: 32 MiB
pieces, above 4,096 bytes only), bu_hip_set_wait_hook, bu_hip_set_stream / bu_hip_get_stream, bu_hip_on_destroy / bu_hip_cancel_on_destroy,
bu_hip_create_context_on / bu_hip_context_device, bu_hip_get_tuning.

Copies are compared byte for byte with the numpy arrays they came from, inside device buffers whose surroundings must keep their fill. Every test that changes a
stream, a hook or tuning does so on a context of its own, closed in a finaliser; the session's context is left alone."""
import ctypes as C
import pathlib

import numpy as np
import pytest

from basis_universal_amd import capi, uastc

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "uastc_reference_vectors.npz"
MIB = 1 << 20
GUARD = 512
HOOK = C.CFUNCTYPE(None, C.c_void_p)


@pytest.fixture
def own_ctx(request):
    made = []

    def make():
        made.append(capi.Context(0))
        return made[-1]
    request.addfinalizer(lambda: [c.close() for c in reversed(made)])
    return make


def pattern(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ----------------------------------------------------------------------------- 1. h2d_async + d2d + d2h

@pytest.mark.parametrize("n", [1, 255, 256, 257, 4 * MIB - 1, 4 * MIB, 4 * MIB + 1, 9 * MIB + 3])
def test_h2d_async_d2d_d2h_single_sizes(own_ctx, n):
    ctx = own_ctx()
    want = pattern(n, n)
    src = want.copy()
    d_a, d_b = ctx.alloc(n + 2 * GUARD), ctx.alloc(n + 2 * GUARD)
    ctx.memset(d_a, 0x5A, n + 2 * GUARD)
    ctx.memset(d_b, 0xC3, n + 2 * GUARD)
    ctx.memcpy_h2d_async(d_a + GUARD, src)
    src[:] = 0   # copied out when the call returns
    ctx.memcpy_d2d(d_b + GUARD, d_a + GUARD, n)   # a consumer right behind the upload, no synchronisation
    b = ctx.download(d_b, (n + 2 * GUARD,), np.uint8)
    a = np.empty(n + 2 * GUARD, np.uint8)
    ctx.memcpy_d2h(a, d_a)
    for got, fill in ((a, 0x5A), (b, 0xC3)):
        assert (got[GUARD:GUARD + n] == want).all(), f"first wrong byte at {np.nonzero(got[GUARD:GUARD + n] != want)[0][:1]}"
        assert (got[:GUARD] == fill).all() and (got[GUARD + n:] == fill).all()
    ctx.free(d_a); ctx.free(d_b)


def test_h2d_async_ring_wraps_under_its_consumers(own_ctx):
    """40 uploads of 1 MiB + 17 bytes through the 16 MiB ring (15 slots of 1 MiB + 256: it wraps twice), each from the same host array, rewritten as soon as the call
    returns, each followed at once by a device copy of its region; one download at the end."""
    ctx = own_ctx()
    n, count = MIB + 17, 40
    d_a, d_b = ctx.alloc(n * count), ctx.alloc(n * count)
    ctx.memset(d_a, 0x5A, n * count)
    ctx.memset(d_b, 0xC3, n * count)
    rng = np.random.default_rng(40)
    want = rng.integers(0, 256, (count, n), dtype=np.uint8)
    src = np.empty(n, np.uint8)
    for k in range(count):
        src[:] = want[k]
        ctx.memcpy_h2d_async(d_a + k * n, src)
        src[:] = 0xEE
        ctx.memcpy_d2d(d_b + k * n, d_a + k * n, n)
    got = ctx.download(d_b, (count, n), np.uint8)
    wrong = [k for k in range(count) if not (got[k] == want[k]).all()]
    assert not wrong, f"uploads {wrong} arrived wrong"
    assert (ctx.download(d_a, (count, n), np.uint8) == want).all()
    ctx.free(d_a); ctx.free(d_b)


# ----------------------------------------------------------------------------- 2. d2h under a wait hook

def test_d2h_under_a_wait_hook(own_ctx):
    ctx = own_ctx()
    sizes = [4096, 4097, MIB + 5, 32 * MIB + 4099]   # the direct path, then the bounce buffer growing; the last one is two pieces
    total = sum(sizes)
    want = pattern(total, 7)
    d = ctx.upload(want)
    calls = [0]

    def count(_user):
        calls[0] += 1
    hook = HOOK(count)
    ctx.set_wait_hook(hook)
    hooked, at = [], 0
    for n in sizes:
        out = np.full(n + GUARD, 0x5A, np.uint8)
        ctx.memcpy_d2h(out[:n], d + at)
        hooked.append(out)
        at += n
    calls_hooked = calls[0]
    scratch = np.zeros(8192, np.uint8)
    assert not ctx.lib.download_begin(ctx.h, scratch.ctypes.data_as(C.c_void_p), d, scratch.nbytes), "download_begin must refuse while a hook is set"
    ctx.set_wait_hook(None)
    calls_at_clear = calls[0]
    plain, at = [], 0
    for n in sizes:
        plain.append(ctx.download(d + at, (n,), np.uint8))
        at += n
    assert calls[0] == calls_at_clear, "the hook ran after it was removed"
    at = 0
    for n, h, p in zip(sizes, hooked, plain):
        for name, got in (("hooked", h[:n]), ("plain", p)):
            assert (got == want[at:at + n]).all(), f"{name} {n}: first wrong byte at {np.nonzero(got != want[at:at + n])[0][:1]}"
        assert (h[n:] == 0x5A).all(), n
        at += n
    # a transfer of 32 MiB is not over by the first look at the stream: the wait went through the hook
    assert calls_hooked > 0
    dl = ctx.lib.download_begin(ctx.h, scratch.ctypes.data_as(C.c_void_p), d, scratch.nbytes)   # available again
    assert dl and ctx.lib.download_wait(dl) == 1 and (scratch == want[:8192]).all()
    ctx.free(d)


# ----------------------------------------------------------------------------- 3. set_stream / get_stream

def test_context_on_another_contexts_stream(own_ctx):
    """A runs on B's stream: what B has enqueued (a 64 MiB fill and copy, then the copy that produces A's tiles) is in front of A's kernels with no event and no host
    wait in between. Back on its own stream A works as before."""
    g = np.load(GOLDEN)
    tiles = np.ascontiguousarray(g["blocks"])
    n = tiles.shape[0]
    a, b = own_ctx(), own_ctx()
    a_own, b_own = a.get_stream(), b.get_stream()
    assert a_own and b_own and a_own != b_own
    big = 64 * MIB
    d_big0, d_big1 = b.alloc(big), b.alloc(big)
    d_stage = b.upload(tiles)
    d_px = b.upload(np.ascontiguousarray(tiles[::-1]))   # other tiles, until the chain below has run
    d_out = b.alloc(n * 16)
    b.memset(d_out, 0xA5, n * 16)
    b.sync()
    a.set_stream(b_own)
    assert a.get_stream() == b_own
    b.memset(d_big0, 3, big)
    b.memcpy_d2d(d_big1, d_big0, big)
    b.memcpy_d2d(d_px, d_stage, n * 64)
    uastc.encode_uastc_blocks(a, d_px, 2, n_blocks=n, out_device=d_out)
    got = a.download(d_out, (n, 16), np.uint8)
    assert (got == g["level2"]).all(), f"{int((got != g['level2']).any(1).sum())} of {n} blocks differ"
    a.set_stream(None)
    assert a.get_stream() == a_own and b.get_stream() == b_own
    b.memset(d_out, 0xA5, n * 16)
    b.sync()
    uastc.encode_uastc_blocks(a, d_px, 0, n_blocks=n, out_device=d_out)
    assert (a.download(d_out, (n, 16), np.uint8) == g["level0"]).all()
    for d in (d_big0, d_big1, d_stage, d_px, d_out):
        b.free(d)


# ----------------------------------------------------------------------------- 4. on_destroy / cancel_on_destroy

def test_destroy_callbacks():
    ran = []
    fn = HOOK(lambda user: ran.append(user))
    other = HOOK(lambda user: ran.append(("other", user)))
    ctx = capi.Context(0)
    try:
        lib, h = ctx.lib, ctx.h
        for user in (1, 2, 3):
            assert lib.on_destroy(h, fn, user) == 1
        assert lib.on_destroy(h, other, 2) == 1
        assert lib.on_destroy(h, None, 4) == 0   # no function: refused
        lib.cancel_on_destroy(h, fn, 2)
        lib.cancel_on_destroy(h, fn, 99)      # unknown pairs: nothing happens
        lib.cancel_on_destroy(h, other, 1)
        assert ran == []
    finally:
        ctx.close()
    assert sorted(ran, key=str) == [("other", 2), 1, 3]
    # the (parked) context comes back without them
    again = capi.Context(0)
    again.close()
    assert len(ran) == 3


# ----------------------------------------------------------------------------- 5. context and tuning queries

def test_context_device_and_bad_device_index(hip_ctx, own_ctx):
    ctx = own_ctx()
    assert ctx.device() == 0 and hip_ctx.device() >= 0
    lib = ctx.lib
    assert lib.context_device(None) == -1
    for bad in (-1, 4096):
        assert not lib.create_context_on(bad)
        assert f"bad device {bad}" in lib.last_error(None)


def test_tuning_round_trip(hip_ctx, own_ctx):
    ctx = own_ctx()
    defaults = hip_ctx.tuning()
    assert ctx.tuning() == defaults
    t = capi.Tuning()
    ctx.lib.get_tuning(None, C.byref(t), C.sizeof(t))   # no context: the process defaults
    assert t.struct_bytes == C.sizeof(t) and {k: getattr(t, k) for k in defaults} == defaults
    changed = dict(tsvq_wide_min=1024, tsvq_wide6_min=0, tsvq_wide_cov_min=5, tsvq_windows=2, tsvq_dense_min=9, tsvq_zero_copy=0, tsvq_chained_only=1, tsvq_poll=1,
                   refine_unsorted=1, debug=0, tsvq_deep_levels=1, uastc_walk_cus=24, codebook_wide_min=77)
    assert set(changed) == set(defaults)
    ctx.set_tuning(**changed)
    assert ctx.tuning() == changed and hip_ctx.tuning() == defaults
    ctx.set_tuning(uastc_walk_cus=8)
    assert ctx.tuning() == dict(defaults, uastc_walk_cus=8)   # fields not named go back to the defaults
    short = capi.Tuning()
    ctx.lib.get_tuning(ctx.h, C.byref(short), 8)   # an older caller's shorter struct: only what fits
    assert (short.struct_bytes, short.tsvq_wide_min, short.tsvq_wide6_min, short.uastc_walk_cus) == (8, defaults["tsvq_wide_min"], 0, 0)
    with pytest.raises(capi.HipError, match="out of range"):
        ctx.set_tuning(tsvq_wide_min=100)
    assert ctx.tuning() == dict(defaults, uastc_walk_cus=8)   # a refused set changes nothing
    ctx.set_tuning()
    assert ctx.tuning() == defaults
