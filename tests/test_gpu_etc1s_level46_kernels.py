"""-m gpu parity tests of the level 4-6 and bookkeeping kernels of the device-resident layer (include/basisu_hip.h section 2): the forced-selector
endpoint refit, the sub-block and backend block errors, the bu_hip_k_map_* index kernels and the multi-GPU shares of the codebook fit.

Every comparison is exact equality. The expected values come from the plain-C oracle (oracle/etc1s_oracle.c, pinned to the real reference in
test_oracle_vs_reference.py) or, for the index kernels, from a few lines of numpy -- never from the code under test. Inputs are OFF the manifold the
frontend produces: random forced selectors, block colours unrelated to the cluster's, lists with duplicates, lists on either side of the 8192-texel
LDS stage, slices that do not start at block 0, planted neighbour patterns.

Every output buffer has SLACK bytes behind it, the whole of it filled with 0xAB before the call: the slack must come back untouched, and so must the
entries a contract leaves alone. Index arrays the kernels read carry in-range padding behind their last entry (said where it is done), so that an
off-by-one shows as a wrong word in the slack instead of a wild read.

Empty lists in bu_hip_k_refit_endpoints_given_selectors: the frontend passes them (a cluster no block uses any more) and skips their results
(etc1s_frontend.cpp: `if (subs.empty() ...) continue`); the kernel touches no texel for them. Their four output entries are unspecified, so one empty
list is passed and nothing is asserted about its entries -- only that its neighbours come out right.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import oracle, ptr, u32p, u64p, csr_from_lists, decode_etc1s_blocks
from dedup_sort_cases import rank_reference as _rank_reference   # sizes, offsets, stable order and positions of a clustering, by numpy
import test_gpu_etc1s_kernels as K

pytestmark = pytest.mark.gpu

VP = C.c_void_p
SLACK = 256
FILL = 0xAB
NONE = 0xFFFFFFFF
Q_MEDIUM, Q_SLOW, Q_UBER = 1, 2, 3
LEVEL_OF_QUALITY = {Q_MEDIUM: 1, Q_SLOW: 2, Q_UBER: 6}   # the compression level whose cluster fit runs at that quality (frontend.cpp:1530-1533)


# ----------------------------------------------------------------------------- buffers with a sentinel

def _out(ctx, nbytes):
    """a device buffer of nbytes + SLACK bytes, all 0xAB"""
    d = ctx.alloc(nbytes + SLACK)
    ctx.check(ctx.lib.memset(ctx.h, d, FILL, nbytes + SLACK), "memset")
    return d


def _fetch(ctx, d, shape, dtype, free=True):
    """the first prod(shape) entries of a buffer made by _out; the SLACK bytes behind them must still hold the sentinel"""
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    raw = ctx.download(d, (nbytes + SLACK,), np.uint8)
    assert (raw[nbytes:] == FILL).all(), f"wrote past the end of a {np.dtype(dtype).name}{list(shape)} output: bytes {np.nonzero(raw[nbytes:] != FILL)[0][:8]} of the slack"
    if free:
        ctx.free(d)
    return raw[:nbytes].copy().view(dtype).reshape(shape)


def _sentinel(shape, dtype):
    return np.full(int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def _upload_padded(ctx, arr, pad_value, pad=16):
    """an input index array with `pad` in-range entries behind its last one"""
    arr = np.ascontiguousarray(arr)
    return ctx.upload(np.concatenate([arr.reshape(-1), np.full(pad, pad_value, arr.dtype)]))


# ----------------------------------------------------------------------------- tiles

def _adversarial_tiles():
    """all-0 and all-255; channels within one intensity-table step of 0 / 255 (some, not all, of a table's colours clamp); single-channel tiles; two far-apart
    colours; solid colours that are exactly 5-bit representable, and solid colours an ETC1S block decodes to exactly (zero error: the optimizer's early out)."""
    rng = np.random.default_rng(46)
    t = []

    def solid(r, g, b):
        a = np.zeros((4, 4, 4), np.uint8); a[..., 0] = r; a[..., 1] = g; a[..., 2] = b
        return a
    t += [solid(0, 0, 0)] * 3 + [solid(255, 255, 255)] * 3
    for step in (2, 5, 8, 9, 17, 29, 42, 60):       # the small and large steps of the first tables
        lo = rng.integers(0, step + 1, (4, 4, 4)).astype(np.uint8)
        t += [lo, (255 - lo).astype(np.uint8)]
        mix = lo.copy(); mix[..., 1] = 255 - lo[..., 1]   # one channel near 255, two near 0
        t.append(mix)
    for c in range(3):
        a = np.zeros((4, 4, 4), np.uint8); a[..., c] = rng.integers(0, 256, (4, 4)); t.append(a)
        a = np.full((4, 4, 4), 255, np.uint8); a[..., c] = rng.integers(0, 256, (4, 4)); t.append(a)
        a = np.zeros((4, 4, 4), np.uint8); a[..., c] = (np.arange(16).reshape(4, 4) * 17); t.append(a)
    for _ in range(8):   # two far-apart colours, split along rows (= along the sub-blocks), columns or at random
        c0, c1 = rng.integers(0, 40, 3), rng.integers(215, 256, 3)
        for mask in (np.arange(16).reshape(4, 4) >= 8, (np.arange(16).reshape(4, 4) % 4) >= 2, rng.integers(0, 2, (4, 4)).astype(bool)):
            a = np.zeros((4, 4, 4), np.uint8); a[..., :3] = np.where(mask[..., None], c1, c0); t.append(a)
    for c5 in ((0, 0, 0), (31, 31, 31), (10, 10, 10), (3, 17, 30), (31, 0, 16), (1, 1, 1)):
        s = [(v << 3) | (v >> 2) for v in c5]
        t.append(solid(*s))                                             # exactly 5-bit representable
        t.append(solid(*[min(v + 2, 255) for v in s]))                  # = colour 2 of table 0 on that base: zero error
        t.append(solid(*[max(v - 17, 0) for v in s]))                   # = colour 0 of table 1
    out = np.ascontiguousarray(np.stack(t))
    out[..., 3] = 255
    return out


def _mix():
    return np.ascontiguousarray(np.concatenate([K._images(), _adversarial_tiles()]))


@pytest.fixture(scope="module")
def mix():
    return _mix()


def _headers(color5_inten):
    """(n, 4) r5, g5, b5, table -> (n, 8) ETC1S blocks with all-zero selector bits (differential, zero deltas, flipped: etc_block::is_etc1s)"""
    p = np.ascontiguousarray(color5_inten, np.uint8).reshape(-1, 4)
    blk = np.zeros((p.shape[0], 8), np.uint8)
    blk[:, 0:3] = p[:, 0:3] << 3
    blk[:, 3] = (p[:, 3] << 5) | (p[:, 3] << 2) | 3
    return blk


def _determine_selectors(blocks, per_block_params, perceptual):
    out = np.zeros((blocks.shape[0], 8), np.uint8)
    oracle().orc_determine_selectors(ptr(blocks), blocks.shape[0], ptr(np.ascontiguousarray(per_block_params)), perceptual, ptr(out))
    return out


# ----------------------------------------------------------------------------- refit with forced selectors

def _refit_case():
    """The tiles (the mix, and the mix with red and blue exchanged: enough sub-blocks for disjoint lists), the lists, and where the empty one sits."""
    m = _mix()
    sw = m.copy(); sw[..., 0] = m[..., 2]; sw[..., 2] = m[..., 0]
    blocks = np.ascontiguousarray(np.concatenate([m, sw]))
    n = blocks.shape[0]
    rng = np.random.default_rng(4646)
    # sub-blocks in the order of their block's luma, cut into runs: colour-coherent lists, as a clustering would give
    by_luma = np.argsort(blocks[..., :3].reshape(n, -1).astype(np.int64).sum(axis=1), kind="stable")
    tv = np.stack([by_luma * 2, by_luma * 2 + 1], axis=1).reshape(-1).astype(np.uint32)
    fixed = [1, 2, 3, 7, 1023, 1024, 1025, 4096]     # 1023 / 1024 / 1025 sub-blocks = 8184 / 8192 / 8200 texels around CB_STAGE; 4096 = 32,768 texels = the default wide_min
    rest = tv.size - sum(fixed)
    assert rest > 2000
    cuts = np.sort(rng.choice(np.arange(1, rest), size=39, replace=False))
    sizes = fixed + [int(s) for s in np.diff(np.concatenate([[0], cuts, [rest]]))]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    lists, at = [], 0
    for s in sizes:
        lists.append(rng.permutation(tv[at:at + s]).astype(np.uint32)); at += s
    assert at == tv.size
    some = rng.permutation(n)[:40].astype(np.uint32)
    lists.append(np.array([some[0] * 2 + 1] * 3 + [some[1] * 2] * 2 + [some[2] * 2, some[2] * 2 + 1, some[2] * 2], np.uint32))   # the same sub-block several times
    grown = max((l for l in lists if len(l) <= 400), key=len)
    lists.append(np.concatenate([grown, grown, grown[:7]]).astype(np.uint32))            # a list that "grew": every entry twice, some three times
    lists.append((some[3:12] * 2 + 1).astype(np.uint32))                                 # lower halves only
    lists.append((some[12:21] * 2).astype(np.uint32))                                    # upper halves only
    two = np.nonzero((blocks[:, 0, 0, :3].astype(np.int64).sum(axis=1) < 130) & (blocks[:, 3, 3, :3].astype(np.int64).sum(axis=1) > 640))[0]   # rows 0-1 dark, rows 2-3 bright
    assert two.size >= 4
    lists.append((two[:8] * 2 + 1).astype(np.uint32)); lists.append((two[:8] * 2).astype(np.uint32))
    empty_at = len(lists) // 2
    lists.insert(empty_at, np.zeros(0, np.uint32))
    assert {0, 1, 2, 3, 7, 1023, 1024, 1025, 4096} <= {len(l) for l in lists}
    return blocks, lists, empty_at


_REFIT = {}


def _refit_inputs():
    if "case" not in _REFIT:
        _REFIT["case"] = _refit_case()
    return _REFIT["case"]


def _refit_encodings(perceptual):
    """(a) the frontend-like encoding: every block under the colours of its cluster of a 300-entry codebook, nearest selectors; (b) the same headers with seeded
    random selector bits, a tenth of the blocks under a colour that has nothing to do with their cluster"""
    key = ("enc", perceptual)
    if key not in _REFIT:
        blocks = _refit_inputs()[0]
        n = blocks.shape[0]
        params, block_cluster = K._codebook(blocks, 300, 11, perceptual=perceptual)
        a = _determine_selectors(blocks, params[block_cluster], perceptual)
        assert (a[:, :4] == _headers(params[block_cluster])[:, :4]).all()
        rng = np.random.default_rng(99 + perceptual)
        per_block = params[block_cluster].copy()
        odd = rng.permutation(n)[:n // 10]
        per_block[odd, :3] = rng.integers(0, 32, (odd.size, 3)); per_block[odd, 3] = rng.integers(0, 8, odd.size)
        b = _headers(per_block)
        b[:, 4:] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        _REFIT[key] = {"a": a, "b": np.ascontiguousarray(b)}
    return _REFIT[key]


def _refit_expected(perceptual, quality, variant):
    key = ("exp", perceptual, quality, variant)
    if key not in _REFIT:
        blocks, lists, _ = _refit_inputs()
        enc = _refit_encodings(perceptual)[variant]
        offs, idx = csr_from_lists(lists)
        k = len(lists)
        params = _sentinel((k, 4), np.uint8); err = _sentinel((k,), np.uint64); valid = _sentinel((k,), np.uint8); cur = _sentinel((k,), np.uint64)
        oracle().orc_refit_endpoints_given_selectors(ptr(blocks), ptr(enc), k, ptr(offs, u32p), ptr(idx, u32p), quality, perceptual, ptr(params), ptr(err, u64p),
                                                     ptr(valid), ptr(cur, u64p))
        _REFIT[key] = (params, err, valid, cur)
    return _REFIT[key]


@pytest.mark.parametrize("wide_min", [None, 8, 0])
@pytest.mark.parametrize("quality", [Q_SLOW, Q_UBER])
@pytest.mark.parametrize("perceptual", [1, 0])
def test_refit_endpoints_given_selectors(hip_ctx, perceptual, quality, wide_min, request):
    """bu_hip_k_refit_endpoints_given_selectors_q (and, at uber quality, the plain form) against orc_refit_endpoints_given_selectors: params, err, valid and the
    lists' current error, per cluster. wide_min as in test_generate_endpoint_codebook: default (only the 4096-sub-block list takes the many-workgroup passes),
    8 (every list does), 0 (none does)."""
    if wide_min is not None:
        request.addfinalizer(hip_ctx.set_tuning)
        hip_ctx.set_tuning(codebook_wide_min=wide_min)
    blocks, lists, empty_at = _refit_inputs()
    offs, idx = csr_from_lists(lists)
    k = len(lists)
    keep = np.arange(k) != empty_at
    kept = np.nonzero(keep)[0]
    L = hip_ctx.lib
    d_blocks, d_offs, d_idx = hip_ctx.upload(blocks), hip_ctx.upload(offs), hip_ctx.upload(idx)
    differs_from_nearest = 0
    for variant in ("a", "b"):
        enc = _refit_encodings(perceptual)[variant]
        exp = _refit_expected(perceptual, quality, variant)
        assert (exp[2][keep] == 1).all()
        d_enc = hip_ctx.upload(enc)
        for form in (("q", "plain") if quality == Q_UBER else ("q",)):
            d_params, d_err, d_valid, d_cur = _out(hip_ctx, k * 4), _out(hip_ctx, k * 8), _out(hip_ctx, k), _out(hip_ctx, k * 8)
            if form == "q":
                hip_ctx.check(L.k_refit_endpoints_given_selectors_q(hip_ctx.h, d_blocks, d_enc, k, offs.ctypes.data_as(VP), d_offs, d_idx, quality, perceptual,
                                                                   d_params, d_err, d_valid, d_cur), "k_refit_q")
            else:
                hip_ctx.check(L.k_refit_endpoints_given_selectors(hip_ctx.h, d_blocks, d_enc, k, offs.ctypes.data_as(VP), d_offs, d_idx, perceptual,
                                                                 d_params, d_err, d_valid, d_cur), "k_refit")
            got = (_fetch(hip_ctx, d_params, (k, 4), np.uint8), _fetch(hip_ctx, d_err, (k,), np.uint64), _fetch(hip_ctx, d_valid, (k,), np.uint8),
                   _fetch(hip_ctx, d_cur, (k,), np.uint64))
            for name, g, e in zip(("params", "err", "valid", "cur_err"), got, exp):
                bad = kept[(g[keep] != e[keep]).reshape(kept.size, -1).any(axis=1)]
                assert bad.size == 0, (f"{name} (encoding {variant}, form {form}): {bad.size} of {kept.size} clusters differ, list sizes {[len(lists[i]) for i in bad[:6]]}: "
                                       f"got {g[bad[:3]].tolist()} exp {e[bad[:3]].tolist()}")
        hip_ctx.free(d_enc)
        if variant == "b":
            # not degenerate: with random selectors the forced fit is not the nearest-colour fit of the same lists, nor is the current error the refit error
            o2, i2 = csr_from_lists([lists[i] for i in kept])
            p = np.zeros((kept.size, 4), np.uint8); e = np.zeros(kept.size, np.uint64); v = np.zeros(kept.size, np.uint8)
            oracle().orc_generate_endpoint_codebook(ptr(blocks), kept.size, ptr(o2, u32p), ptr(i2, u32p), LEVEL_OF_QUALITY[quality], perceptual, 0, ptr(p), ptr(e, u64p), ptr(v))
            differs_from_nearest = int((e != exp[1][keep]).sum())
            assert (exp[3][keep] != exp[1][keep]).any(), "current error equals the refit error everywhere"
    assert differs_from_nearest > 0, "the forced fit equals the nearest-colour fit on every list: the test is degenerate"
    for q in (d_blocks, d_offs, d_idx):
        hip_ctx.free(q)


# ----------------------------------------------------------------------------- sub-block errors

@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("n_blocks", [1, 127, 128, 129, 3520])
def test_subblock_errors(hip_ctx, mix, n_blocks, perceptual):
    """bu_hip_k_subblock_errors against orc_subblock_errors (the reference's unscaled-colour quirk included): 2 n_blocks around the 256 sub-blocks of a workgroup,
    cluster colours with 5-bit values 0 and 31 under intensity tables 0 and 7."""
    rng = np.random.default_rng(n_blocks)
    blocks = np.ascontiguousarray(mix[rng.permutation(mix.shape[0])[:n_blocks]])
    corners = [(0, 0, 0, 0), (0, 0, 0, 7), (31, 31, 31, 0), (31, 31, 31, 7), (0, 31, 0, 0), (31, 0, 31, 7), (0, 0, 31, 3), (16, 16, 16, 7)]
    k = 64
    params = np.ascontiguousarray(np.concatenate([np.array(corners, np.uint8),
                                                  np.concatenate([rng.integers(0, 32, (k - 8, 3)), rng.integers(0, 8, (k - 8, 1))], axis=1).astype(np.uint8)]))
    block_cluster = rng.integers(0, k, n_blocks).astype(np.uint32)
    block_cluster[:min(8, n_blocks)] = np.arange(8)[:n_blocks]
    block_cluster[-1] = 3
    exp = np.zeros(2 * n_blocks, np.uint64)
    oracle().orc_subblock_errors(ptr(blocks), n_blocks, ptr(block_cluster, u32p), ptr(params), perceptual, ptr(exp, u64p))
    d_blocks, d_bc, d_prm = hip_ctx.upload(blocks), hip_ctx.upload(block_cluster), hip_ctx.upload(params)
    d_out = _out(hip_ctx, 2 * n_blocks * 8)
    hip_ctx.check(hip_ctx.lib.k_subblock_errors(hip_ctx.h, d_blocks, n_blocks, d_bc, d_prm, perceptual, d_out), "k_subblock_errors")
    got = _fetch(hip_ctx, d_out, (2 * n_blocks,), np.uint64)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{bad.size} of {2 * n_blocks} sub-blocks differ, first {bad[:6]}: got {got[bad[:6]]} exp {exp[bad[:6]]}"
    # the quirk is visible in this input: scaled colours would give other errors
    scaled = params.copy(); scaled[:, :3] = (params[:, :3] << 3) | (params[:, :3] >> 2)
    other = np.zeros(2 * n_blocks, np.uint64)
    oracle().orc_subblock_errors(ptr(blocks), n_blocks, ptr(block_cluster, u32p), ptr(scaled), perceptual, ptr(other, u64p))
    assert (other != exp).any()
    for q in (d_blocks, d_bc, d_prm):
        hip_ctx.free(q)


# ----------------------------------------------------------------------------- backend block errors

def _backend_case(mix, nbx, nby, seed):
    """Two slices of nbx x nby blocks back to back. Clusters are distinct per block except for planted repeats, so that most interior slots carry a number; every rule
    that blanks a slot is planted at a known place where the grid has room for it. The endpoint table has total + 4 entries and EVERY block's index lies inside it; the
    call is told n_clusters = total, so the four highest indices are "out of range" for the entry point while no read can leave the table."""
    rng = np.random.default_rng(seed)
    per = nbx * nby
    total = 2 * per
    assert total <= mix.shape[0]
    blocks = np.ascontiguousarray(mix[rng.permutation(mix.shape[0])[:total]])
    etc = np.zeros((total, 8), np.uint8)
    oracle().orc_encode_etc1s_blocks(ptr(blocks), total, 1, 1, ptr(etc))
    etc[::2, 4:] = rng.integers(0, 256, (etc[::2].shape[0], 4), dtype=np.uint8)    # half of the blocks: selectors the colours did not choose
    n_clusters = total
    cluster = rng.permutation(total).astype(np.uint32)          # distinct, all < n_clusters
    # the table: a cluster's endpoints = the header of the block that owns it (r5, g5, b5, table), random for the four spare entries
    hdr = np.stack([etc[:, 0] >> 3, etc[:, 1] >> 3, etc[:, 2] >> 3, etc[:, 3] >> 5], axis=1).astype(np.uint8)
    table = np.zeros((total + 4, 4), np.uint8)
    table[cluster] = hdr
    table[total:, :3] = rng.integers(0, 32, (4, 3)); table[total:, 3] = rng.integers(0, 8, 4)
    planted = {"equal_left": [], "equal_up": [], "equal_diag": [], "zero": [], "high": []}
    for s in range(2):
        first = s * per

        def at(x, y):
            return first + y * nbx + x
        if nbx >= 5 and nby >= 3:
            if per < 100:   # little room: a fixed layout in which no plant is the source of another
                plan = [("high", (1, 1)), ("zero", (3, 1)), ("equal_up", (4, 1)), ("equal_diag", (1, 2)), ("equal_left", (3, 2))]
            else:           # seeded spots at least three apart, two of each kind
                spots = [(x, y) for y in range(1, nby) for x in range(1, nbx - 1)]
                spots = [spots[i] for i in rng.permutation(len(spots))]
                plan = []
                for kind in ("high", "zero", "equal_left", "equal_up", "equal_diag") * 2:
                    xy = next(c for c in spots if all(max(abs(c[0] - o[0]), abs(c[1] - o[1])) > 2 for _, o in plan))
                    plan.append((kind, xy))
            for kind, (x, y) in plan:
                if kind == "high":
                    cluster[at(x, y)] = n_clusters + int(rng.integers(0, 4))
                elif kind != "zero":
                    dx, dy = {"equal_left": (-1, 0), "equal_up": (0, -1), "equal_diag": (-1, -1)}[kind]
                    cluster[at(x, y)] = cluster[at(x + dx, y + dy)]
                planted[kind].append(at(x, y))
        elif per > 1:    # a single row or column: left-only or upper-only neighbours
            cluster[first + 4] = cluster[first + 3]; planted["equal_left" if nby == 1 else "equal_up"].append(first + 4)
            planted["zero"].append(first + per - 1)
            cluster[first + 1] = n_clusters + 1; planted["high"].append(first + 1)
    for b in planted["zero"]:   # the tile becomes what its block decodes to: zero error whatever the selectors are
        blocks[b, :, :, :3] = decode_etc1s_blocks(etc[b:b + 1], 1, 1)
    return blocks, etc, cluster, table, n_clusters, planted


@pytest.mark.parametrize("with_neighbours", [1, 0])
@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("nbx,nby", [(1, 1), (1, 9), (9, 1), (5, 3), (17, 9)])
def test_backend_block_errors(hip_ctx, mix, nbx, nby, perceptual, with_neighbours):
    """bu_hip_k_backend_block_errors against orc_backend_block_errors for first_block 0 and first_block = one slice further on, one call per slice into fresh
    sentinel-filled outputs: the entries are indexed by absolute block, the other slice's must keep the sentinel (and with_neighbours = 0 must leave d_neighbour_err alone)."""
    blocks, etc, cluster, table, n_clusters, planted = _backend_case(mix, nbx, nby, 100 * nbx + nby)
    per, total = nbx * nby, 2 * nbx * nby
    fill32 = int(_sentinel((1,), np.uint32)[0])
    L = hip_ctx.lib
    d_blocks, d_etc, d_cluster, d_table = hip_ctx.upload(blocks), hip_ctx.upload(etc), hip_ctx.upload(cluster), hip_ctx.upload(table)
    for first in (0, per):
        exp_own = _sentinel((total,), np.uint32); exp_nb = _sentinel((total, 3), np.uint32)
        oracle().orc_backend_block_errors(ptr(blocks), ptr(etc), ptr(cluster, u32p), ptr(table), first, nbx, nby, n_clusters, perceptual, with_neighbours,
                                          ptr(exp_own, u32p), ptr(exp_nb, u32p))
        # what the oracle alone must show: every planted rule fired, and the test is not vacuous
        assert (exp_own[:first] == fill32).all() and (exp_own[first + per:] == fill32).all()
        if with_neighbours:
            assert (exp_nb[:first] == fill32).all() and (exp_nb[first + per:] == fill32).all()
            x, y = np.arange(per) % nbx, np.arange(per) // nbx
            nb = exp_nb[first:first + per]
            assert (nb[x == 0][:, [0, 2]] == NONE).all() and (nb[y == 0][:, [1, 2]] == NONE).all()                       # edge
            here = lambda kinds: [b for kind in kinds for b in planted[kind] if first <= b < first + per]
            equal, zero, high = here(("equal_left", "equal_up", "equal_diag")), here(("zero",)), here(("high",))
            assert all((exp_nb[b] == NONE).all() and exp_own[b] != 0 for b in equal)                                     # ANY neighbour equal: all three blank
            assert all(exp_own[b] == 0 and (exp_nb[b] == NONE).all() for b in zero)                                      # zero error
            for b in high:                                                                                               # index >= n_clusters: blank in the blocks it is a neighbour of
                i = b - first
                for p, (dx, dy) in enumerate(((1, 0), (0, 1), (1, 1))):   # b is the left / upper / upper-left neighbour of the block at (+dx, +dy)
                    if x[i] + dx < nbx and y[i] + dy < nby:
                        assert exp_nb[b + dy * nbx + dx, p] == NONE
            if per > 1:
                assert equal and zero and high
            if nbx >= 5 and nby >= 3:
                assert all(planted[kind] for kind in planted)
                interior = nb[(x > 0) & (y > 0)]
                assert (interior != NONE).sum() * 3 >= interior.size, "fewer than a third of the interior slots carry a number"
                assert any(exp_nb[b + 1, 0] == NONE and (exp_nb[b + 1, 1:] != NONE).any() for b in high)                 # ... while that block's other slots keep theirs
        else:
            assert (exp_nb == fill32).all()
        d_own, d_nb = _out(hip_ctx, total * 4), _out(hip_ctx, total * 12)
        hip_ctx.check(L.k_backend_block_errors(hip_ctx.h, d_blocks, d_etc, d_cluster, d_table, first, nbx, nby, n_clusters, perceptual, with_neighbours, d_own, d_nb),
                      "k_backend_block_errors")
        got_own, got_nb = _fetch(hip_ctx, d_own, (total,), np.uint32), _fetch(hip_ctx, d_nb, (total, 3), np.uint32)
        bad = np.nonzero(got_own != exp_own)[0]
        assert bad.size == 0, f"own error, first_block {first}: blocks {bad[:8]} got {got_own[bad[:8]]} exp {exp_own[bad[:8]]}"
        bad = np.nonzero((got_nb != exp_nb).any(axis=1))[0]
        assert bad.size == 0, f"neighbour errors, first_block {first}: blocks {bad[:6]} got {got_nb[bad[:6]].tolist()} exp {exp_nb[bad[:6]].tolist()}"
    for q in (d_blocks, d_etc, d_cluster, d_table):
        hip_ctx.free(q)


# ----------------------------------------------------------------------------- bookkeeping maps, against numpy

def _cluster_maps():
    rng = np.random.default_rng(2024)
    cases = []
    for n in (1, 255, 256, 257, 100003):
        k = max(3, min(n // 3, 700))
        c = rng.integers(1, k - 1, n).astype(np.uint32) if k > 3 else np.ones(n, np.uint32)      # the first and the last cluster stay empty
        if n > 300:
            c[c == 5] = 6; c[c == 11] = 12                                                     # empty ones in the middle, too
        cases.append((f"n{n}_first_last_empty", c, k))
    cases.append(("one_cluster", np.zeros(1000, np.uint32), 1))
    cases.append(("all_in_one_of_many", np.full(777, 4, np.uint32), 9))
    cases.append(("every_cluster_used", rng.permutation(np.arange(4096, dtype=np.uint32) % 513).astype(np.uint32), 513))
    return cases


_MAPS = _cluster_maps()


@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("case", range(len(_MAPS)), ids=[c[0] for c in _MAPS])
def test_map_rank_blocks_and_endpoint_csr(hip_ctx, case, with_pos):
    _, cluster, k = _MAPS[case]
    n = cluster.size
    L = hip_ctx.lib
    sizes, offsets, order, pos = _rank_reference(cluster, k)
    for c in range(0, k, max(1, k // 50)):
        assert (np.diff(order[offsets[c]:offsets[c + 1]].astype(np.int64)) > 0).all()    # ascending inside every list (the numpy reference itself)
    d_cluster = hip_ctx.upload(cluster)
    d_sizes, d_offsets, d_sorted = _out(hip_ctx, (k + 1) * 4), _out(hip_ctx, (k + 1) * 4), _out(hip_ctx, n * 4)
    d_pos = _out(hip_ctx, n * 4) if with_pos else None
    hip_ctx.check(L.k_map_rank_blocks(hip_ctx.h, d_cluster, n, k, d_sizes, d_offsets, d_sorted, d_pos), "k_map_rank_blocks")
    assert (_fetch(hip_ctx, d_sizes, (k + 1,), np.uint32) == sizes).all()
    assert (_fetch(hip_ctx, d_offsets, (k + 1,), np.uint32) == offsets).all()
    assert (_fetch(hip_ctx, d_sorted, (n,), np.uint32) == order).all()
    if with_pos:
        assert (_fetch(hip_ctx, d_pos, (n,), np.uint32) == pos).all()
        # map_endpoint_csr on the result: offsets in training-vector units. Behind their last entry the two per-block inputs describe the block that WOULD come next
        # in the last cluster, so a thread one past the end lands in the output's slack.
        d_cl = _upload_padded(hip_ctx, cluster, k - 1); d_ps = _upload_padded(hip_ctx, pos, sizes[k - 1])
        d_o2 = hip_ctx.upload((offsets * 2).astype(np.uint32))
        d_idx = _out(hip_ctx, 2 * n * 4)
        hip_ctx.check(L.k_map_endpoint_csr(hip_ctx.h, d_cl, d_ps, n, d_o2, d_idx), "k_map_endpoint_csr")
        want = np.stack([order * 2, order * 2 + 1], axis=1).reshape(-1).astype(np.uint32)
        assert (_fetch(hip_ctx, d_idx, (2 * n,), np.uint32) == want).all()
        for q in (d_cl, d_ps, d_o2):
            hip_ctx.free(q)
    hip_ctx.free(d_cluster)


@pytest.mark.parametrize("optional", ["both", "no_base", "no_pos", "neither"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_map_remap(hip_ctx, n, optional):
    """cluster[b] = new_index[old], pos[b] += base[old] when both pos and base are given. The two arrays are rewritten in place, so what lies behind their last entry
    is an in-range value (not 0xAB) that a remap would change: a thread one past the end shows there."""
    rng = np.random.default_rng(n)
    k = 37
    cluster = rng.integers(0, k, n).astype(np.uint32); pos = rng.integers(0, 1000, n).astype(np.uint32)
    new_index = rng.integers(0, 20, k).astype(np.uint32); base = rng.integers(1, 5000, k).astype(np.uint32)
    new_index[k - 1] = 19
    use_pos, use_base = optional in ("both", "no_base"), optional in ("both", "no_pos")
    d_cluster, d_pos = _upload_padded(hip_ctx, cluster, k - 1), _upload_padded(hip_ctx, pos, 7)
    d_new, d_base = hip_ctx.upload(new_index), hip_ctx.upload(base)
    hip_ctx.check(hip_ctx.lib.k_map_remap(hip_ctx.h, d_cluster, d_pos if use_pos else None, n, d_new, d_base if use_base else None), "k_map_remap")
    got_c, got_p = hip_ctx.download(d_cluster, (n + 16,), np.uint32), hip_ctx.download(d_pos, (n + 16,), np.uint32)
    assert (got_c[:n] == new_index[cluster]).all() and (got_c[n:] == k - 1).all()
    assert (got_p[:n] == (pos + base[cluster] if use_pos and use_base else pos)).all() and (got_p[n:] == 7).all()
    for q in (d_cluster, d_pos, d_new, d_base):
        hip_ctx.free(q)


@pytest.mark.parametrize("differing", ["none", "one", "last", "all", "some"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000003])
def test_map_count_differences(hip_ctx, n, differing):
    """n == 0: the entry point clears the count and returns without a launch."""
    rng = np.random.default_rng(n + 1)
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    b = a.copy()
    if n:
        if differing == "one":
            b[n // 2] ^= np.uint32(1)
        elif differing == "last":
            b[n - 1] ^= np.uint32(0x80000000)
        elif differing == "all":
            b ^= np.uint32(1)
        elif differing == "some":
            b[rng.integers(0, n, max(1, n // 7))] += np.uint32(3)
    d_a, d_b = hip_ctx.upload(a), hip_ctx.upload(b)
    d_count = _out(hip_ctx, 4)
    hip_ctx.check(hip_ctx.lib.k_map_count_differences(hip_ctx.h, d_a, d_b, n, d_count), "k_map_count_differences")
    assert int(_fetch(hip_ctx, d_count, (1,), np.uint32)[0]) == int((a != b).sum())
    hip_ctx.free(d_a); hip_ctx.free(d_b)


@pytest.mark.parametrize("with_parent", [True, False])
@pytest.mark.parametrize("n", [1, 256, 257, 20000])
def test_map_membership(hip_ctx, n, with_parent):
    rng = np.random.default_rng(n + 5)
    parents, k = (5 if with_parent else 1), 301
    cluster = rng.integers(0, k, n).astype(np.uint32)
    cluster[cluster == 0] = 1; cluster[cluster == k - 1] = 2; cluster[-1] = k - 2
    parent = (cluster % parents).astype(np.uint8) if with_parent else None
    want = np.zeros((parents, k), np.uint8)
    want[parent if with_parent else 0, cluster] = 1
    d_cluster = hip_ctx.upload(cluster); d_parent = hip_ctx.upload(parent) if with_parent else None
    d_flags = _out(hip_ctx, parents * k)
    hip_ctx.check(hip_ctx.lib.k_map_membership(hip_ctx.h, d_parent, d_cluster, n, parents, k, d_flags), "k_map_membership")
    assert (_fetch(hip_ctx, d_flags, (parents, k), np.uint8) == want).all()
    hip_ctx.free(d_cluster)
    if with_parent:
        hip_ctx.free(d_parent)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_map_gather(hip_ctx, n):
    """n == 0: returns before the launch; the output keeps its sentinel."""
    rng = np.random.default_rng(n + 9)
    table = rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)
    index = rng.integers(0, 1000, n).astype(np.uint32)
    if n:
        index[0] = 999; index[-1] = 0
    d_table, d_index = hip_ctx.upload(table), _upload_padded(hip_ctx, index, 500)
    d_out = _out(hip_ctx, n * 4)
    hip_ctx.check(hip_ctx.lib.k_map_gather(hip_ctx.h, d_table, d_index, n, d_out), "k_map_gather")
    assert (_fetch(hip_ctx, d_out, (n,), np.uint32) == table[index]).all()
    hip_ctx.free(d_table); hip_ctx.free(d_index)


@pytest.mark.parametrize("optional", ["all", "no_pos", "no_parent", "parent_out_only", "cluster_only"])
@pytest.mark.parametrize("n", [1, 257, 3520])
def test_map_blocks_from_groups(hip_ctx, mix, n, optional):
    """Groups = the output of bu_hip_k_unique_endpoint_vectors (itself held to the oracle in test_gpu_etc1s_kernels.py; here its group structure is checked with numpy
    before it is used): every block of distinct vector u gets cluster leaf[u], position first_pos[u] + its rank in the group, parent parent_of[u]."""
    rng = np.random.default_rng(n)
    L = hip_ctx.lib
    etc = np.zeros((n, 8), np.uint8)
    oracle().orc_encode_etc1s_blocks(ptr(np.ascontiguousarray(mix[:n])), n, 1, 1, ptr(etc))
    d_etc = hip_ctx.upload(etc)
    d_idx, d_keys, d_goffs = hip_ctx.alloc((n + 16) * 4), hip_ctx.alloc(n * 8 + 8), hip_ctx.alloc((n + 1) * 4 + 8)
    u = C.c_uint32(0)
    hip_ctx.check(L.k_unique_endpoint_vectors(hip_ctx.h, d_etc, n, d_idx, d_keys, d_goffs, C.byref(u)), "k_unique_endpoint_vectors")
    ut = u.value
    assert 1 <= ut <= n
    goffs, idx = hip_ctx.download(d_goffs, (ut + 1,), np.uint32), hip_ctx.download(d_idx, (n,), np.uint32)
    assert goffs[0] == 0 and goffs[ut] == n and (np.diff(goffs.astype(np.int64)) > 0).all() and (np.sort(idx) == np.arange(n)).all()
    # behind the last sorted block id: block n, which is the first entry of every output's slack
    pad = np.full(16, n, np.uint32)
    hip_ctx.check(L.memcpy_h2d(hip_ctx.h, d_idx + n * 4, pad.ctypes.data_as(VP), pad.nbytes), "h2d")
    leaf = rng.integers(0, 50, ut).astype(np.uint32); first_pos = rng.integers(0, 100000, ut).astype(np.uint32); parent_of = rng.integers(0, 256, ut).astype(np.uint32)
    group = np.repeat(np.arange(ut), np.diff(goffs.astype(np.int64)))         # group of sorted position j
    rank = (np.arange(n) - goffs[group]).astype(np.uint32)
    want_cluster = np.zeros(n, np.uint32); want_cluster[idx] = leaf[group]
    want_pos = np.zeros(n, np.uint32); want_pos[idx] = first_pos[group] + rank
    want_parent = np.zeros(n, np.uint8); want_parent[idx] = parent_of[group].astype(np.uint8)
    use_pos = optional in ("all", "no_parent")
    use_parent_in, use_parent_out = optional in ("all", "no_pos"), optional in ("all", "no_pos", "parent_out_only")
    d_leaf, d_first, d_parent_of = hip_ctx.upload(leaf), hip_ctx.upload(first_pos), hip_ctx.upload(parent_of)
    d_cluster, d_pos, d_parent = _out(hip_ctx, n * 4), _out(hip_ctx, n * 4), _out(hip_ctx, n)
    hip_ctx.check(L.k_map_blocks_from_groups(hip_ctx.h, d_goffs, d_idx, n, ut, d_leaf, d_first if use_pos else None, d_parent_of if use_parent_in else None,
                                             d_cluster, d_pos if use_pos else None, d_parent if use_parent_out else None), "k_map_blocks_from_groups")
    assert (_fetch(hip_ctx, d_cluster, (n,), np.uint32) == want_cluster).all()
    got_pos, got_parent = _fetch(hip_ctx, d_pos, (n,), np.uint32), _fetch(hip_ctx, d_parent, (n,), np.uint8)
    assert (got_pos == (want_pos if use_pos else _sentinel((n,), np.uint32))).all()
    if use_parent_out:
        assert (got_parent == (want_parent if use_parent_in else 0)).all()     # no per-vector parents: one parent, 0
    else:
        assert (got_parent == FILL).all()
    for q in (d_etc, d_idx, d_keys, d_goffs, d_leaf, d_first, d_parent_of):
        hip_ctx.free(q)


def test_map_calls_on_nothing(hip_ctx):
    """n == 0 where the entry point returns before any launch (bookkeeping_kernels.hip: `if (!n) return hipSuccess`): success, outputs untouched."""
    L = hip_ctx.lib
    d = [_out(hip_ctx, 64) for _ in range(4)]
    d_in = hip_ctx.upload(np.zeros(16, np.uint32))
    hip_ctx.check(L.k_map_rank_blocks(hip_ctx.h, d_in, 0, 5, d[0], d[1], d[2], d[3]), "k_map_rank_blocks")
    hip_ctx.check(L.k_map_endpoint_csr(hip_ctx.h, d_in, d_in, 0, d_in, d[0]), "k_map_endpoint_csr")
    hip_ctx.check(L.k_map_remap(hip_ctx.h, d[0], d[1], 0, d_in, d_in), "k_map_remap")
    hip_ctx.check(L.k_map_blocks_from_groups(hip_ctx.h, d_in, d_in, 0, 0, d_in, d_in, d_in, d[0], d[1], d[2]), "k_map_blocks_from_groups")
    for q in d:
        assert (_fetch(hip_ctx, q, (64,), np.uint8) == FILL).all()
    hip_ctx.free(d_in)


# ----------------------------------------------------------------------------- the shares of a codebook fit

@pytest.mark.parametrize("step", [0, 1])
@pytest.mark.parametrize("parts", [1, 2, 3, 8])
def test_generate_endpoint_codebook_part(hip_ctx, mix, parts, step):
    """bu_hip_k_generate_endpoint_codebook_part: share `part` = the clusters at positions part, part + parts, ... of the size-descending order (ties in index order).
    One call per part into fresh buffers: entries outside the share keep what they held (the sentinel; for step 1 the previous endpoints and flags, which the share's
    clusters are READ from, so they cannot be the sentinel), and the union over the parts is the one-call result = the oracle's."""
    rng = np.random.default_rng(31)
    blocks = np.ascontiguousarray(mix)
    lists, _ = K._clusters_by_luma(blocks, 61, rng)
    lists += [lists[3][:16].copy(), lists[7][:16].copy(), lists[9][:16].copy(), lists[4][:2].copy(), lists[8][:2].copy()]    # ties in size
    k = len(lists)
    offs, idx = csr_from_lists(lists)
    order = np.argsort(-np.diff(offs.astype(np.int64)), kind="stable")
    O, L = oracle(), hip_ctx.lib
    if step == 0:
        start = (_sentinel((k, 4), np.uint8), _sentinel((k,), np.uint64), _sentinel((k,), np.uint8))
    else:   # the previous codebook, half of it perturbed so that "keep" and "take" both occur, one entry invalid; the errors still the sentinel
        p0 = np.zeros((k, 4), np.uint8); e0 = np.zeros(k, np.uint64); v0 = np.zeros(k, np.uint8)
        O.orc_generate_endpoint_codebook(ptr(blocks), k, ptr(offs, u32p), ptr(idx, u32p), 1, 1, 0, ptr(p0), ptr(e0, u64p), ptr(v0))
        p0[::2, 0] = np.minimum(p0[::2, 0] + 1, 31); p0[1::4, 3] = (p0[1::4, 3] + 1) % 8; v0[5] = 0
        start = (p0, _sentinel((k,), np.uint64), v0)
    exp = tuple(a.copy() for a in start)
    O.orc_generate_endpoint_codebook(ptr(blocks), k, ptr(offs, u32p), ptr(idx, u32p), 1, 1, step, ptr(exp[0]), ptr(exp[1], u64p), ptr(exp[2]))
    if step:
        assert (exp[1] == start[1]).any() and (exp[1] != start[1]).any()    # both branches of keep-unless-better
    d_blocks, d_offs, d_idx = hip_ctx.upload(blocks), hip_ctx.upload(offs), hip_ctx.upload(idx)

    def call(part, n_parts):
        d = [_out(hip_ctx, a.nbytes) for a in start]
        for q, a in zip(d, start):
            hip_ctx.check(L.memcpy_h2d(hip_ctx.h, q, a.ctypes.data_as(VP), a.nbytes), "h2d")
        hip_ctx.check(L.k_generate_endpoint_codebook_part(hip_ctx.h, d_blocks, k, offs.ctypes.data_as(VP), d_offs, d_idx, Q_MEDIUM, 1, step, d[0], d[1], d[2], part, n_parts),
                      "k_generate_endpoint_codebook_part")
        return _fetch(hip_ctx, d[0], (k, 4), np.uint8), _fetch(hip_ctx, d[1], (k,), np.uint64), _fetch(hip_ctx, d[2], (k,), np.uint8)

    union = tuple(a.copy() for a in start)
    for part in range(parts):
        share = np.zeros(k, bool); share[order[part::parts]] = True
        got = call(part, parts)
        for name, g, s, e, un in zip(("params", "err", "valid"), got, start, exp, union):
            assert (g[~share] == s[~share]).all(), f"{name}: part {part} of {parts} touched clusters {np.nonzero((g != s).reshape(k, -1).any(axis=1) & ~share)[0][:8]} outside its share"
            assert (g[share] == e[share]).all(), f"{name}: part {part} of {parts} differs from the oracle in clusters {np.nonzero((g != e).reshape(k, -1).any(axis=1) & share)[0][:8]}"
            un[share] = g[share]
    for un, e in zip(union, exp):
        assert (un == e).all()
    whole = call(0, 1)
    for w, e in zip(whole, exp):
        assert (w == e).all()
    for q in (d_blocks, d_offs, d_idx):
        hip_ctx.free(q)
