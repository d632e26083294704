"""The cases of the ETC1S -> BC7 chroma-filter tests, built from seeds so that the golden file (tests/golden/etc1s_bc7_filter_vectors.npz, written by
tools/gen_golden_etc1s_bc7_filter.py) stores only answers for the tiles and only the files for the states. Two kinds:

tile classes (tile_classes()): (n, 16, 4) u8 RGBA tiles for the mode-5 encoder alone (bu_hip_k_bc7_mode5_tiles against the reference's encode_bc7_mode_5_block), each
class aimed at one route or one comparison of the encoder;
states (states()): synthetic ETC1S states -- endpoint palette, selector palette, per-block indices, slice list -- that this package's backend writer turns into .basis
files, each aimed at one gate of the filter or at its clamped neighbourhood.

Everything the builders claim about their cases (routes, boundary values) is asserted by tests/test_etc1s_bc7_filter_host.py on the CPU restatement."""
import functools
import math
import pathlib

import numpy as np

import etc1s_texture_helpers as X
import etc1s_transcode_helpers as E
import native_libs

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "etc1s_bc7_filter_vectors.npz"
F = np.float32
N_RANDOM = 8192


@functools.lru_cache(maxsize=None)
def golden():
    return native_libs.load_npz_golden(GOLDEN)


# ---------------------------------------------------------------- tiles

def _rgba(rgb):
    rgb = np.asarray(rgb)
    assert rgb.min() >= 0 and rgb.max() <= 255, (rgb.min(), rgb.max())
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def random_tiles(seed, n=N_RANDOM):
    """uniform random pixels, alpha included: the encoder must not look at it"""
    return np.random.default_rng(seed).integers(0, 256, (n, 16, 4), dtype=np.uint8)


def few_colour_tiles(seed, n=4096):
    rng = np.random.default_rng(seed)
    colours = rng.integers(0, 256, (n, 4, 3))
    k = rng.integers(2, 5, n)
    pick = rng.integers(0, 4, (n, 16)) % k[:, None]
    return _rgba(colours[np.arange(n)[:, None], pick])


def equal_tiles(seed):
    """the 256 greys, then 256 seeded colours, every pixel of a tile the same"""
    c = np.concatenate([np.repeat(np.arange(256)[:, None], 3, 1), np.random.default_rng(seed).integers(0, 256, (256, 3))])
    return _rgba(np.repeat(c[:, None, :], 16, 1))


def _four_squares(v):
    """four squares of 0..7 that add up to v, or None"""
    for a in range(min(7, math.isqrt(v)), -1, -1):
        for b in range(min(a, math.isqrt(v - a * a)), -1, -1):
            for c in range(min(b, math.isqrt(v - a * a - b * b)), -1, -1):
                d = math.isqrt(v - a * a - b * b - c * c)
                if d <= c and a * a + b * b + c * c + d * d == v:
                    return [a, b, c, d]
    return None


def deviations(rng, sum_sq):
    """16 integer deviations, each within +-7 and their sum within +-7, whose squares add up to exactly sum_sq (at most 400, so that the draw has room): random squares while more than four
    places are left, then a four-square decomposition of the rest; the signs alternate against the running sum. A channel `base + deviations` then has the integer
    mean `base` under the encoder's (total + 8) >> 4, and its entry of the integer covariance is sum_sq."""
    assert 0 <= sum_sq <= 400
    tail = None
    while tail is None:
        terms, rem = [], sum_sq
        while rem and len(terms) < 12:   # a term no smaller than what keeps the rest within 49 per place left
            need = max(rem - (15 - len(terms)) * 49, 1)
            d = int(rng.integers(math.isqrt(need - 1) + 1, min(7, math.isqrt(rem)) + 1))
            terms.append(d)
            rem -= d * d
        tail = _four_squares(rem)   # None for the few remainders that four squares of at most 7 cannot make: draw again
    terms = sorted(terms + tail, reverse=True) + [0] * (12 - len(terms))
    out, run = [], 0
    for d in terms:
        d = -d if run > 0 else d
        run += d
        out.append(d)
    assert len(out) == 16 and abs(run) <= 7 and sum(d * d for d in out) == sum_sq
    return np.array(out)


def variance_tiles(seed, targets):
    """one tile per target: the largest diagonal entry of its integer covariance is exactly the target, the two other channels' are drawn at or below it"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(targets), 16, 3), np.int64)
    for n, target in enumerate(targets):
        sums = [int(target), int(rng.integers(0, target + 1)), int(rng.integers(0, target + 1))]
        for c, k in enumerate(rng.permutation(3)):
            out[n, :, k] = int(rng.integers(16, 240)) + rng.permutation(deviations(rng, sums[c]))
    return _rgba(out)


def zero_axis_tiles(seed, n_each=32):
    """Two channels anti-correlated with the same spread, the third constant: the covariance makes all three components of the power iteration exactly 0, so the
    encoder falls back to its default axis 306 / 601 / 117. All three pairings."""
    rng = np.random.default_rng(seed)
    out = np.zeros((3 * n_each, 16, 3), np.int64)
    for n in range(3 * n_each):
        a, b, c = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][n // n_each]
        d = rng.permutation(deviations(rng, int(rng.integers(160, 401)))) * int(rng.integers(1, 9))
        base = rng.integers(64, 192, 3)
        out[n, :, a], out[n, :, b], out[n, :, c] = base[a] + d, base[b] - d, base[c]
    return _rgba(out)


def tie_tiles(seed, n=512):
    """Two channels anti-correlated with the same spread, the third on two values, eight pixels each, that do not correlate with the others: the power iteration leaves
    an axis along the third channel alone, so the eight pixels of each value share a dot while they differ widely in the two other channels, and the pixel's number in
    the low four bits decides which of them becomes an endpoint: lowest pixel for the minimum, highest for the maximum."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 16, 3), np.int64)
    for t in range(n):
        a, b, c = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][t % 3]
        v0 = int(rng.integers(8, 180))
        v1 = v0 + int(rng.integers(4, 64))
        half = rng.integers(1, 8, 4)
        half = np.concatenate([half, -half])                    # eight deviations that sum to 0 in each group of eight pixels: nothing correlates
        places = rng.permutation(16)
        d, third = np.zeros(16, np.int64), np.zeros(16, np.int64)
        d[places[:8]], d[places[8:]] = rng.permutation(half), rng.permutation(half)
        third[places[:8]], third[places[8:]] = v0, v1
        scale = int(rng.integers(2, 9))
        base = rng.integers(64, 192, 3)
        out[t, :, a], out[t, :, b], out[t, :, c] = base[a] + d * scale, base[b] - d * scale, third
    return _rgba(out)


def extreme_tiles(seed, n=2048):
    """channels at 0 and 255, with a few values between"""
    rng = np.random.default_rng(seed)
    v = rng.choice([0, 255, 0, 255, 1, 254, 128], (n, 16, 3))
    return _rgba(v)


def midpoint8(i):
    """the 8-bit value halfway between 7-bit endpoints i and i + 1 (always whole): to_7 decides it by one float comparison"""
    return (X.from_7(i) + X.from_7(i + 1)) // 2


def midpoint_tiles(seed):
    """Per midpoint of to_7 two tiles whose channels take only the values (m - 1, m) and (m, m + 1): low variance, so the endpoints are to_7 of exactly these values."""
    rng = np.random.default_rng(seed)
    out = np.zeros((254, 16, 3), np.int64)
    for i in range(127):
        for k in range(2):
            lo = midpoint8(i) - 1 + k
            tile = lo + rng.integers(0, 2, (16, 3))
            tile[0], tile[1] = lo, lo + 1   # both values in every channel
            out[2 * i + k] = tile
    return _rgba(out)


def singular_tiles(seed, n=192):
    """Aimed at the singular least-squares system (every pixel the same weight although the variance is high): two channels anti-correlated with the same spread, as
    in zero_axis_tiles, and the third on two adjacent values that to_7 sends to the same endpoint, balanced so that it does not correlate with the others. The power
    iteration then leaves an axis along the third channel alone; the two pixels at its ends are chosen to agree in the other two channels, the endpoints coincide, and
    every weight is 2. Whether a candidate gets there is the restatement's to say (test_etc1s_bc7_filter_host.py counts them)."""
    rng = np.random.default_rng(seed)
    pairs = [(v, v + 1) for v in range(1, 254) if X.to_7_from_8(v) == X.to_7_from_8(v + 1)]
    out = np.zeros((n, 16, 3), np.int64)
    for t in range(n):
        a, b, c = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][t % 3]
        v0, v1 = pairs[int(rng.integers(len(pairs)))]
        half = rng.integers(2, 8, 4)
        half = np.concatenate([half, -half])                    # eight deviations that sum to 0: each group of eight pixels gets them, so nothing correlates
        places = rng.permutation(16)
        low_group, high_group = np.sort(places[:8]), np.sort(places[8:])   # the pixels on v0 and on v1
        d, third = np.zeros(16, np.int64), np.zeros(16, np.int64)
        d[low_group] = np.concatenate([half[:1], rng.permutation(half[1:])])            # the lowest pixel of the low group and the highest of the high group: the
        d[high_group] = np.concatenate([rng.permutation(half[1:]), half[:1]])           # ends under the tie rule, with the same deviation
        third[low_group], third[high_group] = v0, v1
        scale = int(rng.integers(2, 9))
        base = rng.integers(64, 192, 3)
        out[t, :, a], out[t, :, b], out[t, :, c] = base[a] + d * scale, base[b] - d * scale, third
    return _rgba(out)


def alt_sums_search(seed=112, most=48, chunks=12, chunk=200000):
    """Tiles that tell the three sums of the power iteration from their unrounded form (each formed in binary64 and rounded once, what fused multiply-adds compute
    up to the last step): about 15 in a million uniform random tiles. Vectorised over seeded chunks: the tiles whose end pixels along the axis change colour under
    the unrounded sums, then those whose block the restatement encodes differently. Too slow for every test run, so the golden stores the tiles found
    (alt_sums_tiles) next to their answers. -> (report, (k, 16, 4) u8)"""
    D, rng, kept, report = np.float64, np.random.default_rng(seed), [], {"tiles": 0, "ends_change": 0, "blocks_change": 0}
    t = X.tables()
    for _ in range(chunks):
        tiles = rng.integers(0, 256, (chunk, 16, 4), dtype=np.uint8)
        px = tiles[..., :3].astype(np.int64)
        d = px - ((px.sum(1) + 8) >> 4)[:, None, :]
        ic = [(d[..., a] * d[..., b]).sum(1) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        mv = np.maximum(np.maximum(ic[0], ic[3]), ic[5])
        ok = mv >= 160
        cov = [v.astype(F) for v in ic]
        sc = F(1.0) / np.maximum(mv, 1).astype(F)
        w = [sc * cov[0], sc * cov[3], sc * cov[5]]
        ends = []
        for unrounded in (False, True):
            if unrounded:
                alt = [(cov[a].astype(D) * w[0].astype(D) + cov[b].astype(D) * w[1].astype(D) + cov[c].astype(D) * w[2].astype(D)).astype(F) for a, b, c in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
            else:
                alt = [cov[a] * w[0] + cov[b] * w[1] + cov[c] * w[2] for a, b, c in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
            k = np.maximum(np.maximum(np.abs(alt[0]), np.abs(alt[1])), np.abs(alt[2]))
            ok &= k >= F(.0000125)
            m = F(2048.0) / np.maximum(k, F(.0000125))
            axis = np.stack([(v * m).astype(np.int64) * 16 for v in alt], 1)
            dots = ((px * axis[:, None, :]).sum(2) & ~0xF) + np.arange(16)[None, :]
            ends.append((dots.argmin(1), dots.argmax(1)))
        at = np.arange(chunk)
        hit = ok & ((px[at, ends[0][0]] != px[at, ends[1][0]]).any(1) | (px[at, ends[0][1]] != px[at, ends[1][1]]).any(1))
        report["tiles"] += chunk
        report["ends_change"] += int(hit.sum())
        for n in np.flatnonzero(hit):
            assert not X.MUTATIONS
            plain = X.encode_mode5(t, px[n])[0]
            X.MUTATIONS.add("alt_fused")
            try:
                changed = X.encode_mode5(t, px[n])[0] != plain
            finally:
                X.MUTATIONS.clear()
            if changed:
                report["blocks_change"] += 1
                if len(kept) < most:
                    kept.append(tiles[n])
    return report, np.array(kept, np.uint8)


TILE_SEEDS = {"random": 101, "few": 102, "equal": 103, "var159": 104, "var160": 105, "simple": 106, "zero_axis": 107, "ties": 108, "extremes": 109, "midpoints": 110,
              "singular": 111}


@functools.lru_cache(maxsize=None)
def tile_classes():
    """name -> (n, 16, 4) u8, in the order of the golden's answers; nobody writes into the arrays"""
    s = TILE_SEEDS
    simple_targets = np.random.default_rng(s["simple"]).integers(1, 160, 2048)
    out = {"random": random_tiles(s["random"]), "few": few_colour_tiles(s["few"]), "equal": equal_tiles(s["equal"]), "var159": variance_tiles(s["var159"], [159] * 96),
           "var160": variance_tiles(s["var160"], [160] * 96), "simple": variance_tiles(s["simple"] + 1000, simple_targets), "zero_axis": zero_axis_tiles(s["zero_axis"]),
           "ties": tie_tiles(s["ties"]), "extremes": extreme_tiles(s["extremes"]), "midpoints": midpoint_tiles(s["midpoints"]), "singular": singular_tiles(s["singular"])}
    for a in out.values():
        a.setflags(write=False)
    return out


SEARCHED_CLASSES = ("alt_sums",)   # their tiles are stored in the golden (alt_sums_search())
TILE_CLASSES = tuple(TILE_SEEDS) + SEARCHED_CLASSES


def tiles_of(name, arrays=None):
    """the tiles of a class: built from its seed, or for a searched class read from the golden (or from `arrays`, the generator's golden in the making)"""
    if name in SEARCHED_CLASSES:
        return (golden()[0] if arrays is None else arrays)[name + "_tiles"]
    return tile_classes()[name]


def restate_tiles(tiles, traces=None):
    """the CPU restatement of the encoder over tiles -> ((n, 16) u8 blocks, the route of each)"""
    t = X.tables()
    out, routes = np.zeros((len(tiles), 16), np.uint8), []
    for n, tile in enumerate(np.asarray(tiles)):
        trace = {}
        (lo, hi), route = X.encode_mode5(t, tile[:, :3], trace)
        out[n] = np.frombuffer(int(lo).to_bytes(8, "little") + int(hi).to_bytes(8, "little"), np.uint8)
        routes.append(route)
        if traces is not None:
            traces.append(trace)
    return out, routes


# ---------------------------------------------------------------- states
# A state: {"endpoints": (k, 4) r5 g5 b5 table, "selectors": (m, 16), "images": [[(endpoint index grid, selector index grid) per mip level] per image]}.

GATE_KINDS = [("cg", 9.75), ("cg", 10.0), ("cg", 10.25), ("cg", 10.5), ("co", 9.0), ("co", 12.0)]   # |Co| differences: 9 and 12 are the reachable ones nearest 10
POSITIONS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
BUSY = [tuple((k + o) % 4 for k in range(16)) for o in range(4)] + [(0, 3, 1, 2, 3, 0, 2, 1, 1, 2, 0, 3, 2, 1, 3, 0), (0, 1, 3, 0, 1, 3, 3, 1, 0, 0, 3, 1, 1, 0, 3, 3)]
QUIET = [(1, 2) * 8, (2, 1) * 8, (1, 1, 2, 2) * 4, (2, 2, 1, 1, 1, 2, 2, 1) * 2, (1, 2, 2, 1, 2, 1, 1, 2, 0, 1, 2, 1, 2, 2, 1, 1), (2, 1, 1, 2, 1, 2, 3, 1, 2, 1, 2, 2, 1, 1, 2, 1)]
PRIMARIES = [(31, 0, 0), (0, 31, 0), (0, 0, 31), (31, 31, 0), (31, 0, 31), (0, 31, 31)]


def _scaled():
    v = np.arange(32)
    r, g, b = np.meshgrid((v << 3) | (v >> 2), (v << 3) | (v >> 2), (v << 3) | (v >> 2), indexing="ij")
    return (r - b) / 2.0, -r / 4.0 + g / 2.0 - b / 4.0   # exact in binary32 as well: quarters of small integers


def _differing(co, cg, centre, kind, value, sign):
    """the base colour nearest `centre` that differs from it by exactly sign * value in Cg or in Co, the other component within the threshold; None where there is none"""
    dco, dcg = co - co[centre], cg - cg[centre]
    mine, other = (dcg, dco) if kind == "cg" else (dco, dcg)
    hits = np.argwhere((mine == sign * value) & (np.abs(other) <= 10))
    return tuple(int(v) for v in hits[np.abs(hits - np.array(centre)).sum(1).argmin()]) if len(hits) else None


@functools.lru_cache(maxsize=None)
def gate_pairs(kinds, shared):
    """{(kind, value, sign): (centre base colour, differing base colour)} for both signs of every kind: the centre nearest mid grey from which the difference is
    reachable -- one centre for all of them where `shared`, else each its own. No single centre reaches all of GATE_KINDS."""
    co, cg = _scaled()
    centres = sorted(((r, g, b) for r in range(4, 28) for g in range(4, 28) for b in range(4, 28)), key=lambda c: sum(abs(v - 16) for v in c))
    cases = [(kind, value, sign) for kind, value in kinds for sign in (1, -1)]
    if shared:
        for centre in centres:
            found = {case: _differing(co, cg, centre, *case) for case in cases}
            if all(found.values()):
                return {case: (centre, d) for case, d in found.items()}
        raise AssertionError("no centre reaches every difference")
    out = {}
    for case in cases:
        out[case] = next((centre, d) for centre in centres for d in [_differing(co, cg, centre, *case)] if d)
    return out


class _Palette:
    def __init__(self):
        self.entries, self.patterns = {}, {}

    def entry(self, e):
        return self.entries.setdefault(tuple(int(v) for v in e), len(self.entries))

    def pattern(self, p):
        return self.patterns.setdefault(tuple(int(v) for v in p), len(self.patterns))

    def state(self, images):
        return {"endpoints": np.array(list(self.entries), np.uint8), "selectors": np.array(list(self.patterns), np.uint8), "images": images}


def _cells(pal, cells, per_row):
    """3x3-block cells side by side: a cell is (centre entry, centre pattern, outer entry, outer pattern, differing position, differing entry, its pattern)"""
    rows = -(-len(cells) // per_row)
    ei, si = np.zeros((rows * 3, per_row * 3), np.int64), np.zeros((rows * 3, per_row * 3), np.int64)
    ei[:], si[:] = pal.entry(cells[0][2]), pal.pattern(cells[0][3])
    for n, (ce, cp, oe, op, (dx, dy), de, dp) in enumerate(cells):
        y, x = 3 * (n // per_row), 3 * (n % per_row)
        ei[y:y + 3, x:x + 3], si[y:y + 3, x:x + 3] = pal.entry(oe), pal.pattern(op)
        ei[y + 1, x + 1], si[y + 1, x + 1] = pal.entry(ce), pal.pattern(cp)
        ei[y + 1 + dy, x + 1 + dx], si[y + 1 + dy, x + 1 + dx] = pal.entry(de), pal.pattern(dp)
    return ei, si


def gate_cells():
    """the cells of gate_state() in layout order: (kind, value, sign, position)"""
    return [(kind, value, sign, pos) for kind, value in GATE_KINDS for sign in (1, -1) for pos in POSITIONS]


def gate_state():
    """Cells whose eight outer blocks share the centre's base colour (so none of them differs from it in chroma) except one, per GATE_KINDS, position and sign. The
    centres use tables 3..7 under patterns of three or four selectors: a luma variance far above 3."""
    found = gate_pairs(tuple(GATE_KINDS), False)
    pal, cells = _Palette(), []
    for n, (kind, value, sign, pos) in enumerate(gate_cells()):
        table = 3 + n % 5
        centre, d = found[(kind, value, sign)]
        cells.append((centre + (table,), BUSY[n % len(BUSY)], centre + (2,), BUSY[(n + 1) % 4], pos, d + (table,), BUSY[(n + 2) % 4]))
    return pal.state([[_cells(pal, cells, 8)]])   # a row of cells is the eight positions of one difference and sign: one centre colour along the row


QUIET_KINDS = (("cg", 10.25), ("cg", 10.5), ("co", 12.0))


def quiet_cells():
    return [(kind, value, sign, pos, base) for base in range(8) for kind, value in QUIET_KINDS for sign in (1, -1)
            for pos in ((-1, -1), (1, -1), (-1, 1), (1, 1))]


def quiet_state():
    """Centres that differ from one corner neighbour by just over 10, on the narrowest table under patterns of selectors 1 and 2 (a few with one texel of 0 or 3): the
    interpolation moves one quadrant a little, and the pixels to encode vary so little that the encoder takes its low-variance route."""
    found = gate_pairs(QUIET_KINDS, True)
    pal, cells = _Palette(), []
    for n, (kind, value, sign, pos, base) in enumerate(quiet_cells()):
        centre, d = found[(kind, value, sign)]
        cells.append((centre + (0,), QUIET[(n + base) % len(QUIET)], centre + (0,), QUIET[n % 4], pos, d + (0,), QUIET[(n + 1) % 4]))
    return pal.state([[_cells(pal, cells, 12)]])


def saturated_palette(pal):
    extra = [(31, 16, 0), (0, 16, 31), (16, 0, 31), (31, 0, 16), (0, 0, 0), (31, 31, 31)]
    return [pal.entry(c + (t,)) for c in PRIMARIES + extra for t in range(8)]


def saturated_state(seed, n_images=4, nb=32):
    """n_images images of nb x nb blocks over a palette of extreme and opposed chroma under all eight tables, random entries and random selectors"""
    rng = np.random.default_rng(seed)
    pal = _Palette()
    entries = np.array(saturated_palette(pal))
    patterns = np.array([pal.pattern(p) for p in rng.integers(0, 4, (96, 16))] + [pal.pattern(p) for p in BUSY])
    return pal.state([[(entries[rng.integers(0, len(entries), (nb, nb))], patterns[rng.integers(0, len(patterns), (nb, nb))])] for _ in range(n_images)])


def _chain(w, h):
    return [(max(w >> k, 1), max(h >> k, 1)) for k in range(max(w, h).bit_length())]


# Whole mip chains, because the reference tool unpacks no others. 36x4 gives 9x1, 5x1, 3x1 blocks and three levels of 1x1; 12x12 gives 3x3, 2x2, 1x1, 1x1; the 2x1 grid
# comes from 8x4.
THIN_CHAINS = {"thin_wide": _chain(36, 4), "thin_tall": _chain(4, 36), "thin_square": _chain(12, 12), "thin_pair": _chain(8, 4), "thin_pair_tall": _chain(4, 8)}


def thin_state(name):
    """a mip chain of THIN_CHAINS whose adjacent blocks alternate between opposed saturated entries: every block of every level is filtered, and every clamped neighbour position occurs"""
    pal = _Palette()
    a, b = [pal.entry(e) for e in ((31, 2, 4, 4), (1, 29, 27, 5))]
    levels = []
    for k, (w, h) in enumerate(THIN_CHAINS[name]):
        nbx, nby = -(-w // 4), -(-h // 4)
        y, x = np.mgrid[0:nby, 0:nbx]
        levels.append((np.where((x + y + k) % 2 == 0, a, b), np.vectorize(lambda v: pal.pattern(BUSY[v % len(BUSY)]))(x * 3 + y * 5 + k)))
    state = pal.state([levels])
    state["sizes"] = [THIN_CHAINS[name]]
    return state


def block_gate(entries, sel):
    """The filter's variance gate for blocks of the endpoint entries (n, 4) under one selector pattern, vectorised over the entries in the restatement's operation order
    -> (the gate value in binary32, the same with mean * mean and the difference formed in binary64 and rounded once, the exact variance times 4096 as an integer).
    Patterns of one selector have no variance and are not for here."""
    t, entries, sel = X.tables(), np.asarray(entries, np.int64), np.asarray(sel, np.int64)
    n = len(entries)
    base = (entries[:, :3] << 3) | (entries[:, :3] >> 2)
    colors = np.clip(base[:, None, :] + E.INTEN[entries[:, 3]][:, :, None], 0, 255)
    used = sorted(set(int(s) for s in sel))
    low, high = used[0], used[-1]
    assert len(used) > 1
    if len(used) == 2:
        l, h = colors[:, low] >> 1, colors[:, high] >> 1
        if int(sel[0]) != low:
            l, h = h, l
        idx = np.broadcast_to(np.where(sel == sel[0], 0, 3), (n, 16))
    else:
        r = X.RANGES.index((low, high))
        rows = [t["bc7_color"][entries[:, 3], entries[:, c], r].astype(np.int64) for c in range(3)]
        m = sum(row >> 16 for row in rows).argmin(1)
        at = np.arange(n)
        l, h = np.stack([row[at, m] & 127 for row in rows], 1), np.stack([(row[at, m] >> 8) & 127 for row in rows], 1)
        idx = np.array(X.MAPPINGS)[m][:, sel]
        swap = (idx[:, 0] & 2) != 0
        l, h, idx = np.where(swap[:, None], h, l), np.where(swap[:, None], l, h), np.where(swap[:, None], idx ^ 3, idx)
    l8, h8 = (l << 1) | (l >> 6), (h << 1) | (h >> 6)
    w = np.array([0, 21, 43, 64])
    c = (l8[:, None, :] * (64 - w)[None, :, None] + h8[:, None, :] * w[None, :, None] + 32) >> 6
    y_vals = c[..., 0].astype(F) * F(.25) + c[..., 1].astype(F) * F(.5) + c[..., 2].astype(F) * F(.25)
    at = np.arange(n)
    y_sum, y_sq = np.zeros(n, F), np.zeros(n, F)
    for i in range(16):
        y = y_vals[at, idx[:, i]]
        y_sum = y_sum + y
        y_sq = y_sq + y * y
    S = F(1.0) / F(16.0)
    mean = y_sum * S
    gate = (y_sq * S) - mean * mean
    fused = ((y_sq * S).astype(np.float64) - mean.astype(np.float64) * mean.astype(np.float64)).astype(F)
    y4 = (c[..., 0] + 2 * c[..., 1] + c[..., 2])[at[:, None], idx]
    return gate, fused, 16 * (y4 * y4).sum(1) - y4.sum(1) ** 2


def _compositions(total, parts):
    if parts == 1:
        return [(total,)]
    return [(k,) + rest for k in range(1, total - parts + 2) for rest in _compositions(total - k, parts - 1)]


@functools.lru_cache(maxsize=None)
def variance_patterns(seed=120):
    """The selector arrangements of the variance search: for each of the six two-selector ranges and of the five sets of three and four selectors, every way to
    share the 16 texels among the selectors (the counts decide the variance), each in one seeded order of the texels (the order decides the rounding of the running
    sums); then BUSY and QUIET."""
    rng = np.random.default_rng(seed)
    out = []
    for used in list(X.RANGES) + [(0, 1, 2), (1, 2, 3), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3)]:
        for counts in _compositions(16, len(used)):
            out.append(tuple(int(v) for v in rng.permutation(np.repeat(used, counts))))
    return out + BUSY + QUIET


def variance_search():
    """Every endpoint entry (8 x 32^3) whose four colours are distinct (the file writer keeps such a block's selectors as they are) under every pattern of
    variance_patterns(): blocks whose gate value lies within 0.05 of 3.0 (near_by_table: most on the narrowest table; on the wide ones only entries that clamp at 255). -> (report, kept): kept = [(entry, pattern index, kind)], kind "exact" where the binary32 gate
    and the exact variance disagree about < 3 (at most 96 kept), "fused" where the unrounded product flips the gate (at most 64), "at3" where the gate value is 3.0
    itself (at most 32), "below" / "above" otherwise, by the side of 3.0 (at most 100 each)."""
    v = np.arange(32)
    grid = np.stack(np.meshgrid(np.arange(8), v, v, v, indexing="ij"), -1).reshape(-1, 4)[:, [1, 2, 3, 0]]
    base = (grid[:, :3] << 3) | (grid[:, :3] >> 2)
    colors = np.clip(base[:, None, :] + E.INTEN[grid[:, 3]][:, :, None], 0, 255)
    grid = grid[(np.diff(colors.sum(2), axis=1) > 0).all(1)]
    patterns = variance_patterns()
    report = {"entries": int(len(grid)), "patterns": len(patterns), "blocks": int(len(grid)) * len(patterns), "near": 0, "exact": 0, "fused": 0, "near_by_table": [0] * 8}
    found = {"below": [], "above": [], "exact": [], "fused": [], "at3": []}
    for p, pat in enumerate(patterns):
        gate, fused, exact = block_gate(grid, pat)
        near = np.abs(gate - F(3.0)) < F(0.05)
        kinds = {"fused": near & ((fused < F(3.0)) != (gate < F(3.0))), "exact": near & ((gate < F(3.0)) != (exact < 3 * 4096))}
        kinds["at3"] = (gate == F(3.0)) & ~kinds["fused"] & ~kinds["exact"]
        rest = near & ~kinds["fused"] & ~kinds["exact"] & ~kinds["at3"]
        kinds["below"], kinds["above"] = rest & (gate < F(3.0)), rest & (gate > F(3.0))
        report["near"] += int(near.sum())
        for table in np.unique(grid[near, 3]):
            report["near_by_table"][int(table)] += int((grid[near, 3] == table).sum())
        for kind in ("fused", "exact", "at3", "below", "above"):
            report[kind] = report.get(kind, 0) + int(kinds[kind].sum())
            found[kind] += [(tuple(int(x) for x in grid[k]), p, kind) for k in np.flatnonzero(kinds[kind])]
    rng = np.random.default_rng(121)
    kept = []
    for kind, most in (("fused", 64), ("exact", 96), ("at3", 32), ("below", 100), ("above", 100)):
        pick = rng.permutation(len(found[kind]))[:most]
        kept += [found[kind][k] for k in sorted(pick)]
    return report, kept


def opposed(entry):
    """a saturated primary whose chroma is more than 20 from the entry's in Co or Cg"""
    co, cg = X.cocg(entry)
    for c in PRIMARIES:
        oc, og = X.cocg(c)
        if abs(oc - co) > 20 or abs(og - cg) > 20:
            far = c
            if abs(oc - co) + abs(og - cg) > 120:
                return c
    return far


def variance_state(kept):
    """the blocks variance_search() kept, each at an even place of a 32-wide grid between solid blocks (one selector: no variance, left alone by the gate) of an
    entry opposed to it in chroma"""
    pal, patterns = _Palette(), variance_patterns()
    nbx = 32
    nby = 2 * -(-len(kept) // (nbx // 2))
    ei, si = np.zeros((nby, nbx), np.int64), np.zeros((nby, nbx), np.int64)
    for n, (entry, p, _) in enumerate(kept):
        y, x = 2 * (n // (nbx // 2)), 2 * (n % (nbx // 2))
        ei[y:y + 2, x:x + 2], si[y:y + 2, x:x + 2] = pal.entry(opposed(entry) + (n % 8,)), pal.pattern((1 + n % 2,) * 16)
        ei[y, x], si[y, x] = pal.entry(entry), pal.pattern(patterns[p])
    return pal.state([[(ei, si)]])


def doubtful_search():
    """The directed search for the encoder's three doubtful routes THROUGH the filter: a saturated primary or a near-primary under every table and under patterns of
    the two low, the two high or all selectors, next to one neighbour that differs by a little more or by much, each cell run through the restatement on its own 3x3
    grid. The rebuilt pixels of a block whose luma varies can only be all equal where every channel clamps. -> (report, cells for _cells())."""
    t = X.tables()
    near = [(30, 1, 0), (1, 30, 1), (0, 2, 30), (29, 31, 2), (31, 3, 29), (2, 29, 31), (31, 31, 31), (0, 0, 0)]
    pats = [(0, 1) * 8, (2, 3) * 8, (0, 0, 1, 1) * 4, (1, 0, 0, 0) * 4, (3, 2, 2, 2) * 4] + BUSY[:2]
    report, cells = {"cells": 0, "equal": 0, "pca_det": 0, "default_axis": 0}, []
    for c in PRIMARIES + near:
        for table in range(8):
            for pat in pats:
                for d in ((max(c[0] - 3, 0), min(c[1] + 3, 31), c[2]), (c[0], max(c[1] - 3, 0), min(c[2] + 3, 31)), (31 - c[0], 31 - c[1], 31 - c[2])):
                    ep = np.array([c + (table,), d + (table,)], np.uint8)
                    ei = np.zeros((3, 3), np.int64)
                    ei[0, 0] = 1
                    lo, hi = X.bc7_color(t, ep[0], pat)
                    trace = {}
                    _, route = X.chroma_filter_block(t, lo, hi, ep, ei, 1, 1, None, trace)
                    report["cells"] += 1
                    hit = "default_axis" if trace.get("default_axis") else (route if route in ("equal", "pca_det") else None)
                    if hit:
                        report[hit] += 1
                        if sum(1 for x in cells if x[7] == hit) < 64:
                            cells.append((c + (table,), pat, c + (table,), pat, (-1, -1), d + (table,), pat, hit))
    return report, cells


def doubtful_state(cells):
    pal = _Palette()
    return pal.state([[_cells(pal, [x[:7] for x in cells], 8)]])


def write_state(state):
    """the state as a .basis file by this package's backend writer (host only). Several images make a 2D array; the levels of an image are its mip chain."""
    ep, sel = state["endpoints"], state["selectors"]
    ei, si, slices, at = [], [], [], 0
    for image, levels in enumerate(state["images"]):
        for level, (e, s) in enumerate(levels):
            nby, nbx = e.shape
            w, h = state["sizes"][image][level] if "sizes" in state else (nbx * 4, nby * 4)
            slices.append((at, nbx, nby, w, h, image, level, 0))
            ei.append(np.asarray(e).reshape(-1))
            si.append(np.asarray(s).reshape(-1))
            at += nbx * nby
    be = E.backend_from_state(ep, sel, np.concatenate(ei), np.concatenate(si), slices)
    try:
        be.encode()
        return np.asarray(be.basis_file(tex_type=1 if len(state["images"]) > 1 else 0), np.uint8).copy()
    finally:
        be.close()


SATURATED_SEED = 130


# ---------------------------------------------------------------- mutations of the restatement
# mutation (etc1s_texture_helpers.MUTATIONS) -> (the tile classes, the states) whose golden blocks the host test searches for a change: the first 512 tiles of a class,
# 4,096 where the mutation shows that rarely. The generator searches everything and writes the counts into the golden's meta.
MUTATIONS = {"chroma_ge": ((), ("gate",)), "var_le": ((), ("variance",)), "var_fused": ((), ("variance",)), "alt_fused": (("alt_sums",), ()), "ls_fused": (("random",), ()),
             "recip": (("random", "few"), ()), "axis_round": (("random",), ()), "to7_ge": (("midpoints",), ()), "skip_corner": ((), ("gate",)),
             "clamp_off": ((), ("thin_wide", "thin_tall", "thin_square")), "tie_other": (("ties", "singular"), ()), "thresh_161": (("var160",), ())}
FIRST_TILES = {"axis_round": 4096}
FILTER_ONLY = ("chroma_ge", "var_le", "var_fused", "skip_corner", "clamp_off")
# var_fused cannot change a block: variance_search() went through every block the gate can see near 3.0 and found none where the unrounded product lands on the
# other side (docs/HISTORY.md 38); the host test holds the golden's record of that search instead.
EQUIVALENT = ("var_fused",)


def blocks_changed(mutation, arrays, everything=False):
    """how many golden blocks the restatement gets wrong with `mutation` switched on -> {tile class or state: count}"""
    from basis_universal_amd.transcode import decode_etc1s_file
    classes, states = MUTATIONS[mutation]
    if everything:
        classes = () if mutation in FILTER_ONLY else TILE_CLASSES
        states = tuple(k[5:] for k in arrays if k.startswith("file_") and (mutation in FILTER_ONLY or k != "file_saturated"))
    out = {}
    assert not X.MUTATIONS
    X.MUTATIONS.add(mutation)
    try:
        for name in classes:
            pick = slice(None, FIRST_TILES.get(mutation, 512)) if not everything else (slice(None, None, 8) if name == "random" else slice(None))
            out[name] = int((restate_tiles(tiles_of(name, arrays)[pick])[0] != arrays["tiles_" + name][pick]).any(1).sum())
        for name in states:
            dec = decode_etc1s_file(arrays["file_" + name])
            out[name] = sum(int((X.bc7_blocks(dec, im, True) != arrays[E.image_key(name, im["level"], im["layer"], im["face"]) + "_bc7"]).any(1).sum()) for im in dec["images"])
    finally:
        X.MUTATIONS.clear()
    return out
