"""Seeded inputs of the UASTC RDO tests whose answer depends on the LAST block of the look-back window (plain module: the CPU tests of the host core and the GPU
tests of the strips kernel build the same cases from it).

On image-shaped input a walk with a window of w blocks and one with w + 1 give all but the same bytes (docs/HISTORY.md, "RDO window tests"), so a kernel that looks
one block too far or too short passes any such test. A period case puts the one good candidate of every tail block exactly P blocks back: under a tight
max_rms_ratio almost only that twin is admitted, and a window of P - 1 blocks and one of P blocks give different bytes in many blocks."""
import functools

import numpy as np

import helpers

PERIOD_PARAMS = dict(lam=10.0, max_rms_ratio=1.2)   # the tight ratio admits almost only the twin
SENSITIVE_MODES = (15, 17, 18)                      # rdo_mode_reads_endpoint_bits: the strips that take the walk with the refit in it
MIN_DIFFERING = 20                                  # blocks in which the two windows of a pair must differ


def make_la(tiles, every):
    """every `every`-th tile luminance + alpha, in place (tests/test_uastc_rdo_host.py, test_host_rdo_vs_reference_random_params)"""
    grey = tiles[::every, :, :, 1].copy()
    tiles[::every, :, :, 0] = grey
    tiles[::every, :, :, 2] = grey
    tiles[::every, :, :, 3] = 255 - grey // 2


@functools.lru_cache(maxsize=None)
def _source_tiles(seed):
    t = helpers.to_pixel_blocks(helpers.synth(384, 256, seed))
    t.setflags(write=False)
    return t


def period_tiles(P, tail, seed, la_every=0):
    """n = P + tail tiles: the first P of synth(384, 256, seed), then tile P + k = tile k of this very sequence (so a tail longer than P goes on in periods) with an
    integer of {-1, 0, 1} added to every colour byte, clipped. With la_every = m every m-th of the first P tiles is luminance + alpha, and so is its twin in the tail:
    there the three colour bytes of a texel take the same integer and alpha follows the grey level, so that the tail keeps blocks of modes 15 / 17 where the window
    has begun to slide."""
    src = _source_tiles(seed)
    assert 0 < P <= src.shape[0] and tail > 0
    tiles = np.concatenate([src[:P], np.zeros((tail, 4, 4, 4), np.uint8)])
    la = np.zeros(P + tail, bool)
    if la_every:
        make_la(tiles[:P], la_every)
        la[:P:la_every] = True
    rng = np.random.default_rng([seed, P, tail])
    noise = rng.integers(-1, 2, size=(tail, 4, 4, 3))
    for k in range(0, tail, P):   # a period at a time: tile P + k needs the finished tile k
        m = min(P, tail - k)
        prev, d = tiles[k:k + m], noise[k:k + m].copy()
        d[la[k:k + m]] = d[la[k:k + m]][..., 1:2]
        nxt = prev.copy()
        nxt[..., :3] = np.clip(prev[..., :3].astype(np.int16) + d, 0, 255).astype(np.uint8)
        nxt[la[k:k + m], :, :, 3] = 255 - nxt[la[k:k + m], :, :, 1] // 2
        tiles[P + k:P + k + m] = nxt
        la[P + k:P + k + m] = la[k:k + m]
    return np.ascontiguousarray(tiles)


@functools.lru_cache(maxsize=None)
def rdo_period_case(P, tail, seed, la_every=0):
    """(packed, blocks), read-only and shared: period_tiles and their level-0 UASTC blocks from the host build of the encoder (pinned to the reference elsewhere).
    Two things are not the plain "tile k plus {-1, 0, 1} on every colour byte": the twin of a luminance-alpha tile takes ONE integer per texel for its three colour
    bytes and its alpha is recomputed from the grey level (with independent noise per byte no tail tile stays in mode 15 / 17), and a tail longer than P goes on in
    periods, tile P + k made from the finished tile k."""
    blocks = period_tiles(P, tail, seed, la_every)
    packed = helpers.host_encode_uastc(blocks, 0)
    blocks.setflags(write=False)
    packed.setflags(write=False)
    return packed, blocks


def modes_of(packed):
    return np.array(helpers.UASTC_HUFF_MODES)[packed[:, 0] & 127]


@functools.lru_cache(maxsize=None)
def period_pair(P, tail, seed, la_every=0, refine=1, table_trials=True):
    """The host core on a period case at w = P - 1 and w = P: ((bytes, counts) short, (bytes, counts) exact), computed once per process."""
    packed, blocks = rdo_period_case(P, tail, seed, la_every)
    out = []
    for w in (P - 1, P):
        got, counts = helpers.host_uastc_rdo_counted(packed, blocks, 0, 0, table_trials, dict_size=16 * w, refine=refine, **PERIOD_PARAMS)
        got.setflags(write=False)
        out.append((got, counts))
    return tuple(out)


def check_condition(P, packed, short, exact, la_every, first=0):
    """The condition every test on a period pair states before it looks at the device: the two windows differ in at least MIN_DIFFERING blocks, all of them in the
    tail, and with luminance-alpha tiles the strip holds a block of a sensitive mode. Returns the differing block indices."""
    diff = np.nonzero((short != exact).any(1))[0]
    assert diff.size >= MIN_DIFFERING, f"P {P}: windows {P - 1} and {P} differ in {diff.size} blocks only"
    assert diff.min() >= first + P, f"P {P}: block {diff.min()} in front of the tail differs"
    if la_every:
        assert np.isin(modes_of(packed), SENSITIVE_MODES).any(), f"P {P}: no block of mode 15 / 17 / 18"
    return diff


@functools.lru_cache(maxsize=None)
def ref_period(P, tail, seed, la_every, refine, w):
    """The reference on a period case at a window of w blocks, computed once per process."""
    packed, blocks = rdo_period_case(P, tail, seed, la_every)
    got = helpers.ref_uastc_rdo(packed, blocks, 0, 0, dict_size=16 * w, refine=refine, **PERIOD_PARAMS)
    got.setflags(write=False)
    return got


# ---- inactive blocks: strips the walk does nothing in, and one in which skipped blocks decide what their neighbours cost

INACTIVE_STRIP = 400
MIN_SHARED_FIELDS = 20


def _opaque(rgb):
    t = np.full(rgb.shape[:3] + (4,), 255, np.uint8)
    t[..., :3] = np.clip(np.rint(rgb), 0, 255)
    return t


@functools.lru_cache(maxsize=None)
def inactive_case(seed=7):
    """(packed, blocks, shared) at level 0, three strips of INACTIVE_STRIP blocks:
      one    uniform-noise tiles: every block is skipped at the default skip_rms
      two    solid tiles (mode 8): they enter the look-back ring but not the history
      three  strict interleave loud, solid, quiet. Quiet tile k has its 16 colours on one line of RGB space at six levels: the active class. Loud tile k is quiet tile k
             with +-26 added at right angles to that line: the projection on the line, hence the selectors, stay what they are in many tiles, while the error the
             single line leaves makes the block a skipped one.
    shared: indices of the quiet blocks whose mode and selector field equal those of the skipped block two in front. The history entry that skipped block leaves
    decides whether the quiet block's own selectors are priced as a match or as literals, and with it the `modified` count."""
    rng = np.random.default_rng(seed)
    n = INACTIVE_STRIP
    noise = rng.integers(0, 256, size=(n, 4, 4, 4), dtype=np.uint8)
    noise[..., 3] = 255
    n3 = (n + 2) // 3
    solid = np.broadcast_to(rng.integers(0, 256, size=(n + n3, 1, 1, 4), dtype=np.uint8), (n + n3, 4, 4, 4))
    c0 = rng.integers(20, 120, size=(n3, 1, 1, 3)).astype(np.float64)
    line = rng.integers(40, 120, size=(n3, 1, 1, 3)).astype(np.float64)
    quiet = c0 + line * (rng.integers(0, 6, size=(n3, 4, 4, 1)) / 5.0)
    side = rng.normal(size=(n3, 1, 1, 3))
    side -= (side * line).sum(-1, keepdims=True) / (line * line).sum(-1, keepdims=True) * line
    side /= np.sqrt((side * side).sum(-1, keepdims=True))
    loud = quiet + side * 26.0 * rng.choice([-1.0, 1.0], size=(n3, 4, 4, 1))
    three = np.zeros((n, 4, 4, 4), np.uint8)
    three[0::3] = _opaque(loud)[:three[0::3].shape[0]]
    three[1::3] = solid[n:][:three[1::3].shape[0]]
    three[2::3] = _opaque(quiet)[:three[2::3].shape[0]]
    blocks = np.ascontiguousarray(np.concatenate([noise, solid[:n], three]))
    packed = helpers.host_encode_uastc(blocks, 0)
    q = np.arange(2 * n + 2, 3 * n, 3)
    mode = modes_of(packed)
    same = (mode[q] == 0) & (mode[q - 2] == 0) & (packed[q, 9:] == packed[q - 2, 9:]).all(1) & ((packed[q, 8] >> 1) == (packed[q - 2, 8] >> 1))   # mode 0: selectors are bits 65..127
    blocks.setflags(write=False)
    packed.setflags(write=False)
    return packed, blocks, q[same]


# ---- what the CPU tests of the host core and the GPU tests of the kernel share

PERIOD_SEED = 41
PERIODS = (5, 257, 2049, 4097)   # window pairs (4, 5): rings of 4 and 8; (256, 257): rings of 256 and 512; (2048, 2049): the largest ring and the HBM build; (4096, 4097): HBM, sliding
PERIOD_TAIL = {5: 60, 257: 257, 2049: 600, 2050: 600, 4097: 303}   # min(P, 600), but: P = 5 twelve periods, so that 20 blocks can differ at all; P = 4097 shortened for time
# (2049, 2050): the smallest window that is read back from HBM must not reach the twin either: what a look-back one block too long at the handover would show up in
PERIODS_PAST_THE_RING = PERIODS + (2050,)
# dictionary sizes that are no multiple of 16, below 16 (the window clamps to one block), and windows that do not fill their ring (3 in 4, 187 in 256, 1250 in 2048) or
# lie one block on either side of the largest ring
DICT_SIZES = (1, 15, 16, 31, 32, 48, 3000, 20000, 32767, 32769)
PARAM_CORNERS = [("literal_cost_0", dict(literal_cost=0)), ("literal_cost_1000", dict(literal_cost=1000)), ("lambda_1e-3", dict(lam=1e-3)), ("lambda_1e4", dict(lam=1e4)),
                 ("ratio_1.0001", dict(max_rms_ratio=1.0001)), ("skip_rms_0", dict(skip_rms=0.0)), ("no_smooth_scale", dict(smooth_scale=1.0, smooth_std_dev=255.0))]
CORNER_BLOCKS = 600   # of the golden blocks, level 2
