"""Test-only helpers of the UASTC transcoder tests: the g++ build of basis_universal_amd/csrc/uastc_transcode.h (tests/native/transcode_host.cpp)."""
import ctypes as C

import numpy as np

import native_libs

u8p = C.POINTER(C.c_uint8)

# transcoder_texture_format values (basis_universal_amd.transcode has the same constants; kept here so the host tests do not need the package's library)
BC1, BC3, BC4, BC5, BC7, ASTC, RGBA32 = 2, 3, 4, 5, 6, 10, 13
BYTES = {BC1: 8, BC3: 16, BC4: 8, BC5: 16, BC7: 16, ASTC: 16, RGBA32: 64}


def transcode_host():
    return native_libs.load("transcode_host")


def _p(a):
    return a.ctypes.data_as(u8p)


def host_transcode(blocks, target, high_quality=False, channels=(0, 3)):
    """-> (per-block output (n, bytes) uint8 -- RGBA32 as (n, 4, 4, 4) --, ok flags (n,) uint8). Refused blocks are zero-filled."""
    L = transcode_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out, ok = np.zeros((n, BYTES[target]), np.uint8), np.zeros(n, np.uint8)
    if target == RGBA32:
        L.ht_rgba32(_p(blocks), n, _p(out), _p(ok))
        return out.reshape(n, 4, 4, 4), ok
    if target == ASTC:
        L.ht_astc(_p(blocks), n, _p(out), _p(ok))
    elif target == BC7:
        L.ht_bc7(_p(blocks), n, _p(out), _p(ok))
    else:
        L.ht_bcn(_p(blocks), n, target, int(high_quality), channels[0], channels[1], _p(out), _p(ok))
    return out, ok


def modes_and_routes(blocks):
    """per block: (mode, 255 for a block the core refuses; BC1 route as bc1_routes has it)"""
    L = transcode_host()
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    modes, routes = np.zeros(blocks.shape[0], np.uint8), np.zeros(blocks.shape[0], np.uint8)
    L.ht_modes_routes(_p(blocks), blocks.shape[0], _p(modes), _p(routes))
    return modes.astype(np.uint32), routes.astype(np.uint32)


def block_modes(blocks):
    return modes_and_routes(blocks)[0]


def bc1_routes(blocks):
    """per block: 0 solid / invalid, otherwise 1 | hint0 << 1 | hint1 << 2"""
    return modes_and_routes(blocks)[1]


def to_raster(tiles, nbx, nby, width, height):
    """(nby * nbx, 4, 4, 4) decoded tiles -> the (height, width, 4) image they cover, cropped"""
    return tiles.reshape(nby, nbx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(nby * 4, nbx * 4, 4)[:height, :width]


# ---------------------------------------------------------------- blocks no encoder writes (tests/golden/uastc_transcode_fuzz.npz)

class Layout:
    """Where the fields of a block of `mode` lie (ht_mode_layout of tests/native/transcode_host.cpp, from the tables the core's unpacker walks)."""

    def __init__(self, mode):
        L = transcode_host()
        a = (C.c_uint32 * 32)()
        L.ht_mode_layout(mode, a)
        a = [int(v) for v in a]
        self.mode, self.code, self.code_len = mode, a[0], a[1]
        self.hint0 = a[3] if a[2] else None
        self.hint1 = a[5] if a[4] else None
        self.pattern_ofs, self.pattern_bits, self.pattern_limit = a[6], a[7], a[8]
        self.ccs_ofs, self.ccs_bits = a[9], a[10]
        self.radix, self.groups_ofs, self.group_bits = a[11], a[13], a[14:14 + a[12]]
        self.ep_ofs, self.ep_bits, self.ep_values, self.per_group = a[22], a[23], a[24], a[25]
        self.weight_ofs, self.weight_len = a[26], a[27]
        self.subsets, self.comps, self.planes, self.weight_bits = a[28], a[29], a[30], a[31]
        self.levels = (self.radix or 1) << self.ep_bits   # endpoint values run 0 .. levels - 1

    def group_fields(self):
        """[(offset, width, first value past what the group's digits can spell: radix ** digits)] of the packed trit / quint groups"""
        out, ofs = [], self.groups_ofs
        for g, nb in enumerate(self.group_bits):
            digits = min(self.per_group, self.ep_values - g * self.per_group)
            out.append((ofs, nb, self.radix ** digits))
            ofs += nb
        return out


_layouts = None


def layouts():
    global _layouts
    if _layouts is None:
        _layouts = [Layout(m) for m in range(19)]
    return _layouts


def code_modes(blocks):
    """the mode the block's leading code names (255: none), whether or not the rest of it is valid"""
    b0 = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.uint32)
    out = np.full(b0.shape[0], 255, np.uint32)
    for lay in reversed(layouts()):   # a lower mode wins, as in the unpacker's scan (the codes are prefix-free, so at most one matches)
        out[(b0 & ((1 << lay.code_len) - 1)) == lay.code] = lay.mode
    return out


def _put(v, ofs, width, value):
    mask = ((1 << width) - 1) << ofs
    return (v & ~mask) | ((int(value) << ofs) & mask)


def _get(v, ofs, width):
    return (v >> ofs) & ((1 << width) - 1)


def _to_blocks(values):
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little") for v in values), np.uint8).reshape(-1, 16).copy()


def _to_ints(blocks):
    return [int.from_bytes(b.tobytes(), "little") for b in np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)]


class _Bits:
    """The raw 64-bit stream of PCG64: the one part of numpy's random module whose output for a seed is promised not to change, which the committed fixture needs."""

    def __init__(self, seed):
        self.g = np.random.PCG64(seed)

    def blocks(self, n):
        return self.g.random_raw(2 * n).astype("<u8").view(np.uint8).reshape(n, 16)

    def bits128(self):
        return int(self.g.random_raw()) | (int(self.g.random_raw()) << 64)

    def below(self, k):
        return int(self.g.random_raw()) % k


def random_bit_blocks(n, seed):
    """n uniformly random 16-byte blocks"""
    return _Bits(seed).blocks(n)


def _random_in_mode(rng, lay):
    """random bits under the mode's code, the pattern index drawn in range: a valid block"""
    v = _put(rng.bits128(), 0, lay.code_len, lay.code)
    if lay.pattern_bits:
        v = _put(v, lay.pattern_ofs, lay.pattern_bits, rng.below(lay.pattern_limit))
    return v


def _put_endpoints(v, lay, values):
    """write all of the block's endpoint values: raw low bits, and the trit / quint digits packed the canonical way"""
    assert len(values) == lay.ep_values and all(0 <= x < lay.levels for x in values)
    for i, x in enumerate(values):
        v = _put(v, lay.ep_ofs + i * lay.ep_bits, lay.ep_bits, x & ((1 << lay.ep_bits) - 1))
    for g, (ofs, nb, limit) in enumerate(lay.group_fields()):
        digits = [x >> lay.ep_bits for x in values[g * lay.per_group:(g + 1) * lay.per_group]]
        packed = sum(d * lay.radix ** k for k, d in enumerate(digits))
        assert packed < limit
        v = _put(v, ofs, nb, packed)
    return v


FAMILIES = ("random", "random_invalid", "hints", "bise_overflow", "degenerate", "solid", "invalid")
INVALID_CAUSES = ("mode code", "2-subset pattern", "3-subset pattern", "mode 7 pattern")
FUZZ_SEED, FUZZ_QUOTA = 20261017, 96
DEGENERATE_KINDS = ("equal", "equal_sum", "all_zero", "all_max", "low_high", "high_low")
# fixture array -> (target, high quality, channels): the nine cases of uastc_transcode_vectors.npz, and the channel selections the reference tool does not show
FUZZ_CASES = {"rgba32": (RGBA32, False, (0, 3)), "astc": (ASTC, False, (0, 3)), "bc7": (BC7, False, (0, 3)), "bc1": (BC1, False, (0, 3)), "bc1_hq": (BC1, True, (0, 3)),
              "bc3": (BC3, False, (0, 3)), "bc3_hq": (BC3, True, (0, 3)), "bc4_r": (BC4, False, (0, 3)), "bc5_ra": (BC5, False, (0, 3)),
              "bc4_g": (BC4, False, (1, 3)), "bc4_b": (BC4, False, (2, 3)), "bc4_a": (BC4, False, (3, 3)), "bc5_gb": (BC5, False, (1, 2))}


def _family_random(rng, quota):
    """uniformly random bits, drawn until each of the 19 modes has `quota` valid blocks; the first `quota` of a mode are kept, and so is every block drawn up to
    that point that does not unpack. -> (valid kept, invalid kept, drawn)"""
    have, kept, bad, drawn = np.zeros(19, np.int64), [], [], 0
    while (have < quota).any():
        assert drawn < 400 * 19 * quota, f"after {drawn} random blocks some mode still has fewer than {quota} valid ones: {have.tolist()} (the rarest is about 1 block in 130)"
        blocks = rng.blocks(1024)
        modes = block_modes(blocks)
        for i in range(blocks.shape[0]):
            drawn += 1
            m = int(modes[i])
            if m == 255:
                bad.append(blocks[i])
            elif have[m] < quota:
                have[m] += 1
                kept.append(blocks[i])
            if (have >= quota).all():
                break
    return np.array(kept, np.uint8), np.array(bad, np.uint8), drawn


def _family_hints(rng, per_setting=16):
    out = []
    for lay in layouts():
        if lay.hint0 is None and lay.hint1 is None:
            continue
        for h0 in (0, 1):
            for h1 in (0, 1):
                for _ in range(per_setting):
                    v = _random_in_mode(rng, lay)
                    if lay.hint0 is not None:
                        v = _put(v, lay.hint0, 1, h0)
                    if lay.hint1 is not None:
                        v = _put(v, lay.hint1, 1, h1)
                    out.append(v)
    return _to_blocks(out)


def _family_bise_overflow(rng, all_ones=8, per_group=4, all_over=8):
    out = []
    for lay in layouts():
        fields = lay.group_fields()
        if not fields:
            continue
        for _ in range(all_ones):
            v = _random_in_mode(rng, lay)
            for ofs, nb, _limit in fields:
                v = _put(v, ofs, nb, (1 << nb) - 1)
            out.append(v)
        for ofs, nb, limit in fields:       # one group past its limit, the first value past it included
            for k in range(per_group):
                out.append(_put(_random_in_mode(rng, lay), ofs, nb, limit if k == 0 else limit + rng.below((1 << nb) - limit)))
        for _ in range(all_over):
            v = _random_in_mode(rng, lay)
            for ofs, nb, limit in fields:
                v = _put(v, ofs, nb, limit + rng.below((1 << nb) - limit))
            out.append(v)
    return _to_blocks(out)


def _degenerate_endpoints(rng, lay, subset, kind):
    """all endpoint values of a block: random, but for `subset` (value 2k of a subset is component k's low end, 2k + 1 its high end)"""
    values = [rng.below(lay.levels) for _ in range(lay.ep_values)]
    base, n = subset * lay.comps * 2, lay.comps
    if kind == "equal":
        for k in range(n):
            values[base + 2 * k + 1] = values[base + 2 * k]
    elif kind == "equal_sum":   # the first two components trade places between the two ends: the ends differ, every sum over components is the same
        a = rng.below(lay.levels)
        b = (a + 1 + rng.below(lay.levels - 1)) % lay.levels
        values[base:base + 4] = [a, b, b, a]
        for k in range(2, n):
            values[base + 2 * k + 1] = values[base + 2 * k]
    else:
        lo, hi = {"all_zero": (0, 0), "all_max": (lay.levels - 1,) * 2, "low_high": (0, lay.levels - 1), "high_low": (lay.levels - 1, 0)}[kind]
        for k in range(n):
            values[base + 2 * k], values[base + 2 * k + 1] = lo, hi
    return values


def _family_degenerate(rng, reps=2):
    out = []
    for lay in layouts():
        if lay.mode == 8:
            continue
        for subset in range(lay.subsets):
            for kind in DEGENERATE_KINDS:
                for weights in ("zero", "ones", "random"):
                    for _ in range(reps):
                        v = _put_endpoints(_random_in_mode(rng, lay), lay, _degenerate_endpoints(rng, lay, subset, kind))
                        if weights != "random":
                            v = _put(v, lay.weight_ofs, lay.weight_len, 0 if weights == "zero" else (1 << lay.weight_len) - 1)
                        out.append(v)
    return _to_blocks(out)


def _family_solid(rng, n=256):
    lay, out = layouts()[8], []
    for i in range(n):
        v = _put(rng.bits128(), 0, lay.code_len, lay.code)
        for c in range(4):
            if i < 16:
                x = 255 * ((i >> c) & 1)
            else:
                pick = rng.below(4)
                x = 0 if pick == 0 else (255 if pick == 1 else rng.below(256))
            v = _put(v, lay.pattern_ofs + 8 * c, 8, x)
        if i % 8 == 7:   # and some with nothing after the colour
            v = _get(v, 0, lay.pattern_ofs + 32)
        out.append(v)
    return _to_blocks(out)


def _family_invalid(rng, per_code=16, per_pattern=3):
    """-> (blocks, cause per block: index into INVALID_CAUSES)"""
    out, cause = [], []
    known = set()
    for lay in layouts():
        known.update(lay.code | (hi << lay.code_len) for hi in range(1 << (7 - lay.code_len)))
    for code in range(128):
        if code not in known:
            for _ in range(per_code):
                out.append(_put(rng.bits128(), 0, 7, code))
                cause.append(0)
    for lay in layouts():
        if not lay.pattern_bits:
            continue
        c = 3 if lay.mode == 7 else (2 if lay.subsets == 3 else 1)
        for pattern in range(lay.pattern_limit, 1 << lay.pattern_bits):
            for _ in range(per_pattern):
                out.append(_put(_random_in_mode(rng, lay), lay.pattern_ofs, lay.pattern_bits, pattern))
                cause.append(c)
    return _to_blocks(out), np.array(cause, np.uint8)


def fuzz_families(seed=FUZZ_SEED, quota=FUZZ_QUOTA):
    """The deterministic block families of tests/golden/uastc_transcode_fuzz.npz -> ({family: (n, 16) uint8}, invalid family's causes, random blocks drawn).
    Every family but `random` / `random_invalid` is built field by field through Layout; each has its own stream, so changing one leaves the others alone."""
    valid, bad, drawn = _family_random(_Bits(seed), quota)
    inv, cause = _family_invalid(_Bits(seed + 5))
    fam = {"random": valid, "random_invalid": bad, "hints": _family_hints(_Bits(seed + 1)), "bise_overflow": _family_bise_overflow(_Bits(seed + 2)),
           "degenerate": _family_degenerate(_Bits(seed + 3)), "solid": _family_solid(_Bits(seed + 4)), "invalid": inv}
    return fam, cause, drawn


def bise_overflow_mask(blocks):
    """per block: some packed trit / quint group of its mode holds a value its digits cannot spell (a trit byte of 243 or more, a quint field of 125 or more, ...)"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    modes, out = code_modes(blocks), np.zeros(blocks.shape[0], bool)
    for i, v in enumerate(_to_ints(blocks)):
        if modes[i] < 19:
            out[i] = any(_get(v, ofs, nb) >= limit for ofs, nb, limit in layouts()[int(modes[i])].group_fields())
    return out


def layout_hints(blocks):
    """per block: hint0 | hint1 << 1 as the mode's layout places them (0 where the mode has no such bit, or the code names no mode)"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    modes, out = code_modes(blocks), np.zeros(blocks.shape[0], np.uint32)
    for i, v in enumerate(_to_ints(blocks)):
        if modes[i] < 19:
            lay = layouts()[int(modes[i])]
            out[i] = (_get(v, lay.hint0, 1) if lay.hint0 is not None else 0) | ((_get(v, lay.hint1, 1) if lay.hint1 is not None else 0) << 1)
    return out


def unpacked_fields(block):
    """what the core's unpacker reads out of one block -> (mode or 255, endpoints, weights, pattern, component selector)"""
    L = transcode_host()
    ep, w, pat, ccs = np.zeros(18, np.uint8), np.zeros(32, np.uint8), C.c_uint32(0), C.c_uint32(0)
    mode = L.ht_unpack(_p(np.ascontiguousarray(block, np.uint8)), _p(ep), _p(w), C.byref(pat), C.byref(ccs))
    return int(mode), ep, w, int(pat.value), int(ccs.value)


def check_fuzz_coverage(blocks, family, valid, invalid_cause, quota):
    """The conditions the fuzz fixture is written under (asserted by tools/gen_golden_uastc_transcode.py before it writes, and by tests/test_uastc_transcode_host.py on the committed file)."""
    ok = valid != 0
    modes = code_modes(blocks)
    per_mode = np.bincount(modes[ok], minlength=19)[:19]
    assert (per_mode >= quota).all(), per_mode
    r = layout_hints(blocks)[ok & (modes != 8)]
    routes = (int(((r & 1) != 0).sum()), int((r == 2).sum()), int((r == 0).sum()))   # hint0 (whatever hint1 says), hint1 only, neither
    assert min(routes) >= 100, routes
    over = bise_overflow_mask(blocks) & ok
    for lay in layouts():
        if lay.group_fields():
            assert (over & (modes == lay.mode)).any(), f"no valid mode {lay.mode} block with a trit / quint group past its radix"
    inv = family == FAMILIES.index("invalid")
    assert not valid[inv].any() and invalid_cause.shape[0] == inv.sum()
    assert (np.bincount(invalid_cause, minlength=4) > 0).all(), invalid_cause
    return per_mode, routes


def assert_equals_reference(blocks, exp_out, exp_ok, got_out, got_ok, what, family=None):
    """Every block compared, none left out: validity flags equal (got_ok None: the caller has none, as the device output), every block the reference accepts byte-equal,
    every block it refuses zero-filled. The message names the family, the mode and the first differing block as hex."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    exp_out, got_out = np.asarray(exp_out).reshape(n, -1), np.asarray(got_out).reshape(n, -1)
    assert exp_out.shape == got_out.shape and exp_ok.shape == (n,), (what, exp_out.shape, got_out.shape)
    names = np.array(FAMILIES)[family] if family is not None else np.full(n, "-")

    def describe(i):
        return (f"block {i} (family {names[i]}, mode {int(code_modes(blocks[i:i + 1])[0])}, reference {'accepts' if exp_ok[i] else 'refuses'}) "
                f"{blocks[i].tobytes().hex()}: got {got_out[i].tobytes().hex()}, reference {exp_out[i].tobytes().hex()}")
    if got_ok is not None:
        bad = np.flatnonzero((np.asarray(got_ok) != 0) != (exp_ok != 0))
        assert bad.size == 0, f"{what}: validity differs on {bad.size} of {n} blocks (families {sorted(set(names[bad]))}); first: {describe(bad[0])}"
    refused = exp_ok == 0
    assert (exp_out[refused] == 0).all(), what
    bad = np.flatnonzero((got_out[refused] != 0).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} refused blocks are not zero-filled; first: {describe(np.flatnonzero(refused)[bad[0]])}"
    bad = np.flatnonzero((got_out != exp_out).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {n} blocks differ (families {sorted(set(names[bad]))}); first: {describe(bad[0])}"
