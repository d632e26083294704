"""-m gpu parity tests of the five blocking, host-pointer entry points of include/basisu_hip.h section 1 (the drop-in for encoder/basisu_opencl.h):
bu_hip_encode_etc1s_blocks, _determine_selectors, _refine_endpoint_clusterization, _find_optimal_selector_clusters_for_each_block, _encode_etc1s_pixel_clusters.

The oracle is oracle/etc1s_oracle.c (pinned to the real reference by tests/test_oracle_vs_reference.py), fed through THIS file's numpy restatement of the
reference's layouts (basisu_opencl.h:37-111, frontend.cpp:1684-1750, 2436-2480) -- never through csrc/host/seam_translate.h, which is the code under test.
Every comparison is bit-exact over every block / cluster; every output buffer lies inside a larger 0xAB-filled array that must come back untouched around it.
The inputs are ones the reference frontend never produces: windows that overlap, nest and share a first offset, clusters filed in two windows, ties between
distinct clusters, a selector_cluster_indices that is no identity, weighted colour lists of every size modulo 8."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import (oracle, ptr, u8p, u32p, u64p, csr_from_lists, etc1s_test_tiles, clusters_by_luma, endpoint_codebook,
                     BU_BLOCK_INFO, BU_ENDPOINT_CLUSTER, BU_FOSC_BLOCK, BU_FOSC_SELECTOR, BU_PIXEL_CLUSTER)

pytestmark = pytest.mark.gpu

VP = C.c_void_p
GUARD = 256
LEVEL_OF_QUALITY = {0: 0, 1: 1, 2: 2, 3: 6}   # the comp_level orc_encode_etc1s_blocks maps to each etc1_optimizer quality (level_to_block_quality)


def quality_of_perms(total_perms):
    """quality_from_perms as include/basisu_hip.h documents it: <= 4 fast, <= 16 medium, <= 64 slow, above that uber"""
    return 0 if total_perms <= 4 else 1 if total_perms <= 16 else 2 if total_perms <= 64 else 3


# ----------------------------------------------------------------------------- plumbing

@functools.lru_cache(maxsize=None)
def _tiles():
    t = etc1s_test_tiles().copy()
    t[101] = t[100]     # two identical consecutive tiles: a "same tile as the previous block" shortcut wrongly taken by the fosc seam would show
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def tiles():
    return _tiles()


@pytest.fixture(scope="module")
def seam():
    """A context of this module's own (the session's shared one keeps no resident tiles), the tiles set ONCE with bu_hip_set_pixel_blocks."""
    from basis_universal_amd import capi
    ctx = capi.Context()
    t = _tiles()
    ctx.check(ctx.lib.set_pixel_blocks(ctx.h, t.shape[0], t.ctypes.data_as(VP)), "set_pixel_blocks")
    s = Seam(ctx, t.shape[0])
    yield s
    ctx.close()


def vp(a):
    return a.ctypes.data_as(VP) if a is not None else None


class Seam:
    """The five entry points over numpy arrays; every output sits between two 0xAB guards that are checked after the call."""

    def __init__(self, ctx, n):
        self.ctx, self.lib, self.h, self.n_all = ctx, ctx.lib, ctx.h, n
        total = C.c_size_t(0)
        self.d_all = self.lib.get_pixel_blocks_device(self.h, C.byref(total))
        assert self.d_all and total.value == n
        self.n = n

    def adopt(self, d_ptr, n):
        """bu_hip_set_pixel_blocks_device + the read-back of bu_hip_get_pixel_blocks_device"""
        assert self.lib.set_pixel_blocks_device(self.h, n, d_ptr) == 1
        total = C.c_size_t(12345)
        assert self.lib.get_pixel_blocks_device(self.h, C.byref(total)) == d_ptr and total.value == n
        self.n = n

    def restore(self):
        self.adopt(self.d_all, self.n_all)

    def _call(self, fn, out_bytes, dtype, shape, args, expect_ok=True):
        big = np.full(out_bytes + 2 * GUARD, 0xAB, np.uint8)
        rc = fn(self.h, *[VP(big.ctypes.data + GUARD) if a is OUT else a for a in args])
        assert (big[:GUARD] == 0xAB).all() and (big[GUARD + out_bytes:] == 0xAB).all(), "wrote outside the output buffer"
        if not expect_ok:
            assert rc == 0 and (big == 0xAB).all(), "a refused call returns 0 and leaves the output untouched"
            err = self.lib.last_error(self.h)
            assert err, "a refused call leaves a text"
            return err
        assert rc == 1, self.lib.last_error(self.h)
        return big[GUARD:GUARD + out_bytes].view(dtype).reshape(shape).copy()

    def encode_blocks(self, perceptual, total_perms, **kw):
        return self._call(self.lib.encode_etc1s_blocks, self.n * 8, np.uint8, (self.n, 8), (OUT, perceptual, total_perms), **kw)

    def determine_selectors(self, color5_inten, perceptual, **kw):
        return self._call(self.lib.determine_selectors, self.n * 8, np.uint8, (self.n, 8), (vp(color5_inten), OUT, perceptual), **kw)

    def refine(self, info, clusters, perceptual, sorted_block_indices=None, **kw):
        return self._call(self.lib.refine_endpoint_clusterization, self.n * 4, np.uint32, (self.n,),
                          (vp(info), clusters.size, vp(clusters), vp(sorted_block_indices), OUT, perceptual), **kw)

    def fosc(self, info, selectors, cluster_indices, perceptual, **kw):
        return self._call(self.lib.find_optimal_selector_clusters_for_each_block, self.n * 4, np.uint32, (self.n,),
                          (vp(info), selectors.size, vp(selectors), vp(cluster_indices), OUT, perceptual), **kw)

    def pixel_clusters(self, clusters, pixels, weights, perceptual, total_perms, total_pixels=None, **kw):
        k = clusters.size
        return self._call(self.lib.encode_etc1s_pixel_clusters, k * 8, np.uint8, (k, 8),
                          (OUT, k, vp(clusters), pixels.shape[0] if total_pixels is None else total_pixels, vp(pixels), vp(weights), perceptual, total_perms), **kw)


OUT = object()   # stands for the guarded output pointer in Seam._call's argument lists


# ----------------------------------------------------------------------------- encode_etc1s_blocks

@functools.lru_cache(maxsize=None)
def _orc_encode(quality, perceptual):
    t = _tiles()
    exp = np.zeros((t.shape[0], 8), np.uint8)
    oracle().orc_encode_etc1s_blocks(ptr(t), t.shape[0], LEVEL_OF_QUALITY[quality], perceptual, ptr(exp))
    return exp


@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("total_perms", [4, 16, 64, 165, 0, 5, 17, 100, 1000])
def test_encode_etc1s_blocks(seam, total_perms, perceptual):
    """the table values {4, 16, 64, 165} and values off it, which take the next quality up (quality_from_perms)"""
    got = seam.encode_blocks(perceptual, total_perms)
    exp = _orc_encode(quality_of_perms(total_perms), perceptual)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {exp.shape[0]} blocks differ, first {bad[:5]}"


# ----------------------------------------------------------------------------- determine_selectors

@functools.lru_cache(maxsize=None)
def _ds_case(perceptual):
    t = _tiles()
    params, block_cluster = endpoint_codebook(t, 64, 3, perceptual=perceptual)
    c5i = np.ascontiguousarray(params[block_cluster])      # bu_color_rgba {r5, g5, b5, a = inten} per block
    c5i[:8] = [(0, 0, 0, 0), (31, 31, 31, 7), (0, 0, 0, 7), (31, 31, 31, 0), (0, 31, 0, 3), (31, 0, 31, 7), (0, 0, 31, 0), (31, 31, 0, 4)]
    exp = np.zeros((t.shape[0], 8), np.uint8)
    oracle().orc_determine_selectors(ptr(t), t.shape[0], ptr(c5i), perceptual, ptr(exp))
    return c5i, exp


@pytest.mark.parametrize("perceptual", [1, 0])
def test_determine_selectors(seam, perceptual):
    c5i, exp = _ds_case(perceptual)
    got = seam.determine_selectors(c5i, perceptual)
    assert (got == exp).all(), np.nonzero((got != exp).any(axis=1))[0][:8]
    assert np.unique(got[:, 4:], axis=0).shape[0] > 100, "degenerate test: hardly any selectors"


# ----------------------------------------------------------------------------- refine_endpoint_clusterization

N_PARENTS = 7


def _refine_layout(kind, k, cluster_parent, block_cluster, n):
    """-> (cluster index of every flat position, [(first, count)] of the windows, window of every block). Lists are ascending inside a parent, parents laid
    end to end (compute_endpoint_clusters_within_each_parent_cluster, frontend.cpp:971-996) -- then bent in ways the frontend never does."""
    members = [np.nonzero(cluster_parent == p)[0] for p in range(N_PARENTS)]
    block_parent = cluster_parent[block_cluster].astype(np.int64)
    if kind in ("plain", "unsorted", "beyond_65535"):
        flat, wins, at = [], [], 0
        for m in members:
            flat.append(m); wins.append((at, m.size)); at += m.size
        block_win = block_parent.copy()
        flat = np.concatenate(flat)
        if kind == "beyond_65535":
            # filler nobody's window covers up to 65,000, then one window of 2,000 entries there: the flat list has 67,000 entries (> 65,535: refine_workspace_bytes
            # returns 0 and the unsorted kernel runs), offsets and counts still fit 16 bits. Every 8th block is filed under the big window; k is 2,000 here.
            flat = np.concatenate([flat, np.arange(65000 - flat.size) % k, np.arange(2000)])
            wins.append((65000, 2000))
            block_win[::8] = len(wins) - 1
        return flat, wins, block_win
    if kind == "shared":
        # "clusters may live in multiple parent clusters" (frontend.cpp:1706): every cluster of parent 3 is ALSO filed under parent 4, at other positions
        members[4] = np.sort(np.concatenate([members[3], members[4]]))
        flat, wins, at = [], [], 0
        for m in members:
            flat.append(m); wins.append((at, m.size)); at += m.size
        return np.concatenate(flat), wins, block_parent
    if kind == "empty_nested":
        # parents end to end as in "plain", with an EMPTY parent between 2 and 3 (its window (first of 3, 0) belongs to no block). Blocks of parent 1 take the
        # window (0, |0| + |1|) that nests parent 0's (0, |0|); every other block of parent 4 takes (first of 3, |3| + |4|), which shares parent 3's first offset
        first = np.concatenate([[0], np.cumsum([m.size for m in members])])
        wins = [(int(first[p]), members[p].size) for p in range(N_PARENTS)]
        wins[1] = (0, members[0].size + members[1].size)
        wins.append((int(first[3]), members[3].size + members[4].size))
        block_win = block_parent.copy()
        odd = np.nonzero(block_parent == 4)[0][1::2]
        block_win[odd] = len(wins) - 1
        return np.concatenate(members), wins, block_win
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _refine_case(kind, perceptual):
    t = _tiles()
    n, k = t.shape[0], 300
    params, block_cluster = endpoint_codebook(t, k, 11, perceptual=perceptual)
    params = params.copy()
    params[10] = params[11]; params[200] = params[150]     # ties between DISTINCT clusters: the lower position wins unless one of them is the block's current cluster
    cluster_parent = (np.arange(k) * N_PARENTS // k).astype(np.uint8)
    if kind == "beyond_65535":
        # 1,700 more clusters: the 300 with a colour component or the table nudged, so that some of them win
        rng = np.random.default_rng(21)
        more = params[np.arange(1700) % k].copy()
        ch = rng.integers(0, 3, 1700)
        more[np.arange(1700), ch] = np.clip(more[np.arange(1700), ch].astype(np.int64) + rng.choice([-1, 1], 1700), 0, 31)
        more[::5, 3] = (more[::5, 3] + 1) % 8
        params = np.ascontiguousarray(np.concatenate([params, more]))
        k = 2000
    flat, wins, block_win = _refine_layout(kind, k, cluster_parent, block_cluster, n)
    flat = flat.astype(np.int64)
    # the reference's layouts, restated: cl_endpoint_cluster_struct per flat position, cl_block_info_struct per block (frontend.cpp:1684-1750)
    clusters = np.zeros(flat.size, BU_ENDPOINT_CLUSTER)
    clusters["unscaled_color"]["r"], clusters["unscaled_color"]["g"], clusters["unscaled_color"]["b"] = params[flat, 0], params[flat, 1], params[flat, 2]
    clusters["etc_inten"] = params[flat, 3]
    clusters["cluster_index"] = flat
    w = np.asarray(wins, np.int64)
    info = np.zeros(n, BU_BLOCK_INFO)
    info["first_cluster_ofs"], info["num_clusters"] = w[block_win, 0], w[block_win, 1]
    info["cur_cluster_index"] = block_cluster
    info["cur_cluster_etc_inten"] = params[block_cluster, 3]
    for b in range(0, n, 97):   # the layout keeps every block's current cluster inside its window
        f, c = wins[block_win[b]]
        assert block_cluster[b] in flat[f:f + c]
    # the oracle in cluster-index space: the windows' cluster indices as candidate lists
    coffs, cidx = csr_from_lists([flat[f:f + c].astype(np.uint32) for f, c in wins])
    exp = np.zeros(n, np.uint32)
    oracle().orc_refine_endpoint_clusterization(ptr(t), n, ptr(block_cluster, u32p), ptr(params), k, len(wins), ptr(coffs, u32p), ptr(cidx, u32p),
                                                ptr(block_win.astype(np.uint8)), perceptual, ptr(exp, u32p))
    return info, clusters, exp, block_cluster


@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("kind", ["plain", "unsorted", "shared", "empty_nested", "beyond_65535"])
def test_refine_endpoint_clusterization(seam, kind, perceptual, request):
    """k = 300 clusters under 7 parents (2,000 and an eighth window for beyond_65535), ascending lists, against orc_refine_endpoint_clusterization in cluster-index space"""
    info, clusters, exp, block_cluster = _refine_case(kind, perceptual)
    if kind == "unsorted":
        request.addfinalizer(seam.ctx.set_tuning)
        seam.ctx.set_tuning(refine_unsorted=1)
    got = seam.refine(info, clusters, perceptual)
    assert (got == exp).all(), f"{int((got != exp).sum())} of {exp.size} differ, first {np.nonzero(got != exp)[0][:8]}"
    assert (got != block_cluster).sum() > 50, "degenerate test: nothing moved"
    if kind == "beyond_65535":
        assert (got >= 300).sum() > 10, "degenerate test: the big window's own clusters never win"
    if kind == "plain":
        # sorted_block_indices only orders the reference's work items (ocl_kernels.cl:1071-1072): NULL above, garbage here, no effect
        garbage = np.random.default_rng(1).integers(0, 2 ** 32, exp.size, dtype=np.uint64).astype(np.uint32)
        assert (seam.refine(info, clusters, perceptual, sorted_block_indices=garbage) == exp).all()


# ----------------------------------------------------------------------------- find_optimal_selector_clusters_for_each_block

def _unpack_selectors(blocks8):
    """(k, 8) etc_blocks -> (k, 16) selectors [y * 4 + x] (etc.h:232-236, as oracle/etc1s_oracle.c unpack_etc1s)"""
    b = np.ascontiguousarray(blocks8, np.uint8).astype(np.uint64)
    lo = (b[:, 4] << np.uint64(24)) | (b[:, 5] << np.uint64(16)) | (b[:, 6] << np.uint64(8)) | b[:, 7]
    to_sel = np.array([2, 3, 1, 0], np.uint32)
    out = np.zeros((b.shape[0], 16), np.uint32)
    for y in range(4):
        for x in range(4):
            bit = np.uint64(x * 4 + y)
            raw = ((lo >> bit) & np.uint64(1)) | (((lo >> (np.uint64(16) + bit)) & np.uint64(1)) << np.uint64(1))
            out[:, y * 4 + x] = to_sel[raw.astype(np.int64)]
    return out


@functools.lru_cache(maxsize=None)
def _fosc_case(perceptual):
    t = _tiles()
    n, k, n_parents = t.shape[0], 64, 5
    c5i, enc = _ds_case(perceptual)
    c5i, enc = c5i.copy(), enc.copy()
    c5i[101, :3] ^= 3; enc[101, :3] ^= 0x18      # tiles 100 and 101 are identical, their endpoints are not: a choice copied from the previous block would be wrong
    rng = np.random.default_rng(9)
    # 64 selector clusters: a few Lloyd rounds over the blocks' selector vectors from seeded picks (an empty cluster takes one block of a large one); their
    # optimized selectors from the oracle
    u = _unpack_selectors(enc).astype(np.float32)
    cen = u[rng.choice(n, k, replace=False)].copy()
    for _ in range(6):
        assign = ((u * u).sum(axis=1)[:, None] - 2.0 * (u @ cen.T) + (cen * cen).sum(axis=1)[None, :]).argmin(axis=1)
        for c in range(k):
            if (assign == c).any():
                cen[c] = u[assign == c].mean(axis=0)
    for c in range(k):
        if not (assign == c).any():
            assign[np.nonzero(assign == np.bincount(assign, minlength=k).argmax())[0][0]] = c
    lists = [np.nonzero(assign == c)[0].astype(np.uint32) for c in range(k)]
    offs, idx = csr_from_lists(lists)
    sel = np.zeros((k, 8), np.uint8)
    oracle().orc_create_optimized_selector_codebook(ptr(t), ptr(enc), k, ptr(offs, u32p), ptr(idx, u32p), perceptual, ptr(sel))
    # the clusters are dealt to the 5 parents by a permutation, so the flat list is in no cluster order and selector_cluster_indices is no identity
    deal = rng.permutation(k)
    cluster_parent = np.zeros(k, np.int64); cluster_parent[deal] = np.arange(k) * n_parents // k
    members = [deal[cluster_parent[deal] == p] for p in range(n_parents)]
    a, b_ = int(members[0][2]), int(members[0][7])
    sel[b_] = sel[a]                                            # two identical selector blocks in one window: a tie, the lower POSITION wins
    members[3] = np.concatenate([members[3], members[1][:4]])   # four selectors present in two windows
    flat = np.concatenate(members).astype(np.int64)
    first = np.concatenate([[0], np.cumsum([m.size for m in members])])
    block_sel = np.zeros(n, np.int64)
    for ci, l in enumerate(lists):
        block_sel[l] = ci
    block_parent = cluster_parent[block_sel]
    block_parent[101] = (block_parent[100] + 1) % n_parents     # ... and neither are their windows
    # fosc_selector_struct: texel p = y * 4 + x at bits [2p, 2p + 2) (frontend.cpp:2462-2464); fosc_block_struct per block
    packed = (_unpack_selectors(sel) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    selectors = np.zeros(flat.size, BU_FOSC_SELECTOR)
    selectors["packed_selectors"] = packed[flat]
    info = np.zeros(n, BU_FOSC_BLOCK)
    for i, ch in enumerate("rgba"):
        info["etc_color5_inten"][ch] = c5i[:, i]
    info["first_selector"] = first[block_parent]
    info["num_selectors"] = [members[p].size for p in block_parent]
    cluster_indices = np.ascontiguousarray(flat.astype(np.uint32))
    # oracle: the same windows as candidate lists of cluster indices; chunk = 1 is its "no shortcut" mode (it divides by chunk)
    coffs, cidx = csr_from_lists([m.astype(np.uint32) for m in members])
    exp = np.zeros(n, np.uint32)
    enc_copy = enc.copy()
    oracle().orc_find_optimal_selector_clusters(ptr(t), ptr(enc_copy), n, ptr(sel), k, n_parents, ptr(coffs, u32p), ptr(cidx, u32p),
                                                ptr(block_parent.astype(np.uint8)), perceptual, 1, ptr(exp, u32p))
    assert exp[100] != exp[101]
    return info, selectors, cluster_indices, exp, (a, b_)


@pytest.mark.parametrize("perceptual", [1, 0])
def test_find_optimal_selector_clusters_for_each_block(seam, perceptual):
    info, selectors, cluster_indices, exp, tie = _fosc_case(perceptual)
    got = seam.fosc(info, selectors, cluster_indices, perceptual)
    assert (got == exp).all(), f"{int((got != exp).sum())} of {exp.size} differ, first {np.nonzero(got != exp)[0][:8]}"
    assert np.unique(exp).size > 32, "degenerate test: hardly any cluster chosen"
    assert tie[1] not in got[info["first_selector"] == 0], "of two identical selector blocks in one window the lower position wins"


FOSC_LONG_WINDOWS = (383, 384, 385, 700)   # either side of the kernel's quad-table threshold (384 candidates), and well past it


@functools.lru_cache(maxsize=None)
def _fosc_long_case(perceptual):
    """Windows of 383 / 384 / 385 / 700 selectors: the seam entry hands the kernel no candidate words, so this is the way to its quad tables (and, in the first window, its
    pair tables) reading the selector blocks through the list. The flat list holds a seeded codebook of 1,100 words (candidate_list_cases.selector_codebook_words over this
    file's tiles) dealt to the windows by permutations, so selector_cluster_indices is no identity; in every window, where blocks find their minimum, the same word again
    1, 64 and 320 positions on (neighbouring lanes; the same lane one and five iterations later) and in the last position a copy of the first: the lower position wins.
    The oracle runs in POSITION space (one selector block per flat position, windows as candidate lists of positions); the answer is selector_cluster_indices of it."""
    import candidate_list_cases as CL
    t = _tiles()
    n = t.shape[0]
    c5i, enc = _ds_case(perceptual)
    rng = np.random.default_rng(29)
    words = np.concatenate(CL.selector_codebook_words(t, enc, perceptual, rng))
    members = [rng.permutation(words.size)[:m] for m in FOSC_LONG_WINDOWS]
    flat = np.concatenate(members).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(FOSC_LONG_WINDOWS)])
    packed_bits = words[flat].copy()                                    # selector word of every flat position (etc_block bit planes)
    block_win = rng.choice(len(members), n, p=[1 / 6, 1 / 6, 1 / 6, 1 / 2])        # half of the blocks under the long window
    err = CL.fosc_errors(t, enc, packed_bits, perceptual)
    later = []                                                          # flat positions that hold a copy of an earlier position of their window
    for w, m in enumerate(FOSC_LONG_WINDOWS):
        f = int(first[w])
        blocks = np.nonzero(block_win == w)[0]
        votes = np.bincount(err[np.ix_(blocks, np.arange(f, f + m))].argmin(axis=1), minlength=m)
        used, spacing = {0, m - 1}, 0
        packed_bits[f + m - 1] = packed_bits[f]; later.append(f + m - 1)
        for k in np.argsort(-votes, kind="stable")[:40]:
            k, d = int(k), (1, 64, 320)[spacing % 3]
            if votes[k] and k not in used and k + d < m and k + d not in used:
                used.update((k, k + d)); spacing += 1
                packed_bits[f + k + d] = packed_bits[f + k]; later.append(f + k + d)
    sel_pos = CL._words_to_blocks(packed_bits)                          # (positions, 8) etc_blocks for the oracle
    packed = (CL.word_selectors(packed_bits).astype(np.uint32) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)   # fosc_selector_struct
    selectors = np.zeros(flat.size, BU_FOSC_SELECTOR)
    selectors["packed_selectors"] = packed
    info = np.zeros(n, BU_FOSC_BLOCK)
    for i, ch in enumerate("rgba"):
        info["etc_color5_inten"][ch] = c5i[:, i]
    info["first_selector"] = first[block_win]
    info["num_selectors"] = np.asarray(FOSC_LONG_WINDOWS)[block_win]
    cluster_indices = np.ascontiguousarray(flat.astype(np.uint32))
    coffs, cidx = csr_from_lists([np.arange(first[w], first[w + 1], dtype=np.uint32) for w in range(len(members))])
    exp_pos = np.zeros(n, np.uint32)
    enc_copy = enc.copy()
    oracle().orc_find_optimal_selector_clusters(ptr(t), ptr(enc_copy), n, ptr(sel_pos), flat.size, len(members), ptr(coffs, u32p), ptr(cidx, u32p),
                                                ptr(block_win.astype(np.uint8)), perceptual, 1, ptr(exp_pos, u32p))
    assert not np.isin(exp_pos, later).any()                            # of equal words the lower position wins
    return info, selectors, cluster_indices, cluster_indices[exp_pos], exp_pos - first[block_win], len(later)


@pytest.mark.parametrize("perceptual", [1, 0])
def test_find_optimal_selector_clusters_long_windows(seam, perceptual):
    info, selectors, cluster_indices, exp, exp_at, n_copies = _fosc_long_case(perceptual)
    got = seam.fosc(info, selectors, cluster_indices, perceptual)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{bad.size} of {exp.size} differ, first {bad[:8]} (windows of {info['num_selectors'][bad[:8]]}): got {got[bad[:8]]} expected {exp[bad[:8]]}"
    assert n_copies >= 4 * 10 and (exp_at >= 384).sum() >= 50 and np.unique(exp).size > 200, "degenerate test: hardly a winner past position 384, or hardly any cluster chosen"


# ----------------------------------------------------------------------------- encode_etc1s_pixel_clusters

def _cluster_texels(t, tv):
    """texels of training vectors block * 2 + subblock: rows 2 * subblock, 2 * subblock + 1 of the block, in raster order (etc.cpp:352-361)"""
    return t[tv >> 1].reshape(-1, 2, 8, 4)[np.arange(tv.size), tv & 1].reshape(-1, 4)


def _weighted(texels):
    """what the reference hands over (frontend.cpp:1380-1470): the distinct colours of a cluster with their multiplicities"""
    u, counts = np.unique(np.ascontiguousarray(texels).view(np.uint32).reshape(-1), return_counts=True)
    return u.view(np.uint8).reshape(-1, 4).copy(), counts.astype(np.uint32)


def _pixel_layout(lists):
    """[(colours, weights)] -> cl_pixel_cluster array, pixels, weights, laid end to end (basisu_opencl.h:53-68)"""
    cl = np.zeros(len(lists), BU_PIXEL_CLUSTER)
    cl["total_pixels"] = [len(w) for _, w in lists]
    cl["first_pixel_index"] = np.concatenate([[0], np.cumsum([len(w) for _, w in lists])[:-1]])
    return cl, np.ascontiguousarray(np.concatenate([c for c, _ in lists])), np.ascontiguousarray(np.concatenate([w for _, w in lists]).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def _exact_lists():
    """the exact regime: 255 * n * reps < 2^24 for every cluster, so the repetition changes neither a float sum nor the argmin -- a mismatch is a kernel bug"""
    t = _tiles()
    tv_lists, _ = clusters_by_luma(t, 97, np.random.default_rng(7))
    lists = []
    for i, tv in enumerate(tv_lists):
        col, w = _weighted(_cluster_texels(t, tv))
        w[0] += (i - int(w.sum())) % 8            # totals cover every residue modulo 8
        lists.append((col, w))
    lists.append(_weighted(_cluster_texels(t, np.arange(t.shape[0] * 2, dtype=np.uint32))))    # all tiles: a multiple of 8, one repeat
    lists.append((np.array([[9, 200, 77, 255]], np.uint8), np.array([1], np.uint32)))           # one colour, weight 1: written out 8 times
    lists.append((np.array([[130, 131, 29, 255]], np.uint8), np.array([4097], np.uint32)))      # solid
    lists.append((np.array([[40, 50, 60, 255], [40, 50, 60, 255], [44, 50, 60, 255]], np.uint8), np.array([3, 6, 2], np.uint32)))   # the same colour listed twice
    lists.append((np.array([[1, 2, 3, 255], [250, 2, 3, 255], [9, 9, 9, 255]], np.uint8), np.array([5, 0, 6], np.uint32)))           # a zero weight inside
    for _, w in lists:
        n = int(w.sum())
        assert 255 * n * (8 // np.gcd(n, 8)) < 2 ** 24
    assert {int(w.sum()) % 8 for _, w in lists} == set(range(8))
    return lists


@functools.lru_cache(maxsize=None)
def _bright_lists():
    """beyond the exact regime: two bright clusters of 20,001 and 66,001 pixels (reps = 8: 160,008 and 528,008 texels, channel sums near 10^8). The repeated list's
    float colour mean is then a sum of ROUNDED adds, and parity with the unrepeated list is a property of the input, not a theorem. Both lists were checked on the CPU with the
    oracle alone before they went in here: orc_etc1_optimize on the list and on its 8-fold repetition gave the same colour5 and table, and 8 times the error, at MEDIUM, SLOW and
    UBER under both metrics (6 of 6 for each list); no candidate input had to be dropped."""
    rng = np.random.default_rng(33)
    lists = []
    for total, m in ((20001, 1500), (66001, 5000)):
        col = np.unique(rng.integers(120, 256, (m, 3), dtype=np.uint8), axis=0)
        col = np.ascontiguousarray(np.concatenate([col, np.full((col.shape[0], 1), 255, np.uint8)], axis=1))
        w = rng.multinomial(total - col.shape[0], np.full(col.shape[0], 1.0 / col.shape[0])).astype(np.uint32) + 1
        assert int(w.sum()) == total
        lists.append((col, w))
    return lists


def _expand(col, w, reps=1):
    return np.tile(np.repeat(np.ascontiguousarray(col).view(np.uint32).reshape(-1), w.astype(np.int64)), reps)


@functools.lru_cache(maxsize=None)
def _orc_fit(which, quality, perceptual):
    """orc_etc1_optimize on the UNREPEATED expanded list of every cluster -> ((k, 4) colour5 + inten, (k,) error)"""
    lists = _exact_lists() if which == "exact" else _bright_lists()
    prm, err = np.zeros((len(lists), 4), np.uint8), np.zeros(len(lists), np.uint64)
    for i, (col, w) in enumerate(lists):
        px = np.ascontiguousarray(_expand(col, w).view(np.uint8))
        c, inten, e = np.zeros(3, np.uint8), C.c_uint32(0), C.c_uint64(0)
        assert oracle().orc_etc1_optimize(ptr(px), px.size // 4, quality, perceptual, ptr(c), C.byref(inten), C.byref(e), None) == 1
        prm[i, :3], prm[i, 3], err[i] = c, inten.value, e.value
    return prm, err


def _check_pixel_clusters(seam, which, total_perms, perceptual):
    lists = _exact_lists() if which == "exact" else _bright_lists()
    quality = max(quality_of_perms(total_perms), 1)          # the cluster fit has no FAST: 4 behaves as 16
    prm, err = _orc_fit(which, quality, perceptual)
    cl, px, w = _pixel_layout(lists)
    got = seam.pixel_clusters(cl, px, w, perceptual, total_perms)
    # the documented block: colour5 in the top five bits of bytes 0-2 with zero deltas, BOTH table fields = inten, diff and flip bits set, selectors zero
    want = np.zeros((len(lists), 8), np.uint8)
    want[:, :3] = prm[:, :3] << 3
    want[:, 3] = (prm[:, 3] << 5) | (prm[:, 3] << 2) | 3
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{which} perms {total_perms} perceptual {perceptual}: clusters {bad[:8]} differ: got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
    # the device layer on the same expansion, built HERE: its error is reps x the oracle's
    reps = np.array([8 // np.gcd(int(x.sum()), 8) for _, x in lists], np.uint64)
    parts = [_expand(c, x, int(r)) for (c, x), r in zip(lists, reps)]
    tv_counts = [p.size // 8 for p in parts]
    words = np.concatenate(parts)
    words = np.ascontiguousarray(np.concatenate([words, np.zeros(-words.size % 16, np.uint32)]))
    offs = np.concatenate([[0], np.cumsum(tv_counts)]).astype(np.uint32)
    idx = np.arange(offs[-1], dtype=np.uint32)
    ctx, k = seam.ctx, len(lists)
    bufs = [ctx.upload(a) for a in (words, offs, idx)]
    d_params, d_err, d_valid = ctx.alloc(k * 4), ctx.alloc(k * 8), ctx.alloc(k)
    ctx.check(ctx.lib.k_generate_endpoint_codebook(ctx.h, bufs[0], k, vp(offs), bufs[1], bufs[2], quality, perceptual, 0, d_params, d_err, d_valid), "k_gec")
    g_prm, g_err, g_valid = ctx.download(d_params, (k, 4), np.uint8), ctx.download(d_err, (k,), np.uint64), ctx.download(d_valid, (k,), np.uint8)
    for p in bufs + [d_params, d_err, d_valid]:
        ctx.free(p)
    assert (g_valid == 1).all() and (g_prm == prm).all()
    assert (g_err == reps * err).all(), np.nonzero(g_err != reps * err)[0][:8]


@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("total_perms", [4, 16, 64, 165])
def test_encode_etc1s_pixel_clusters(seam, total_perms, perceptual):
    _check_pixel_clusters(seam, "exact", total_perms, perceptual)


@pytest.mark.parametrize("wide_min", [None, 0])
@pytest.mark.parametrize("perceptual", [1, 0])
@pytest.mark.parametrize("total_perms", [16, 64, 165])
def test_encode_etc1s_pixel_clusters_beyond_exact_sums(seam, total_perms, perceptual, wide_min, request):
    """_bright_lists (its docstring has the oracle-against-oracle check these inputs passed). Expanded, both clusters pass bu_hip_tuning::codebook_wide_min (32,768 texels)
    and are fitted by many workgroups (etc1s_codebook_wide.inc); wide_min = 0 sends them through the one-workgroup kernel instead."""
    if wide_min is not None:
        request.addfinalizer(seam.ctx.set_tuning)
        seam.ctx.set_tuning(codebook_wide_min=wide_min)
    _check_pixel_clusters(seam, "bright", total_perms, perceptual)


# ----------------------------------------------------------------------------- ragged runs, caller-owned tiles

@pytest.mark.parametrize("n", [1, 33, 95])
def test_ragged_runs(seam, tiles, n, request):
    """the first n resident tiles (n no multiple of any workgroup's share, and 1): every tile-based entry point, outputs guarded"""
    request.addfinalizer(seam.restore)
    seam.adopt(seam.d_all, n)
    assert (seam.encode_blocks(1, 16) == _orc_encode(1, 1)[:n]).all()
    c5i, exp = _ds_case(1)
    assert (seam.determine_selectors(np.ascontiguousarray(c5i[:n]), 1) == exp[:n]).all()
    info, clusters, exp, _ = _refine_case("empty_nested", 1)
    assert (seam.refine(np.ascontiguousarray(info[:n]), clusters, 1) == exp[:n]).all()
    info, selectors, cluster_indices, exp, _ = _fosc_case(1)
    assert (seam.fosc(np.ascontiguousarray(info[:n]), selectors, cluster_indices, 1) == exp[:n]).all()
    # ... and n pixel clusters
    lists = _exact_lists()[:n]
    prm, _ = _orc_fit("exact", 1, 1)
    got = seam.pixel_clusters(*_pixel_layout(lists), 1, 16)
    assert (got[:, :3] >> 3 == prm[:len(lists), :3]).all() and (got[:, 3] >> 5 == prm[:len(lists), 3]).all()


def test_caller_owned_device_tiles(seam, tiles, request):
    """bu_hip_set_pixel_blocks_device: the entry points over tiles in the caller's own device buffer (here the tile set back to front, so that they are told apart
    from the context's copy); bu_hip_get_pixel_blocks_device hands back the same pointer and count"""
    n = tiles.shape[0]
    rev = np.ascontiguousarray(tiles[::-1])
    d = seam.ctx.upload(rev)
    request.addfinalizer(lambda: (seam.restore(), seam.ctx.free(d)))
    seam.adopt(d, n)     # asserts pointer and count
    assert (seam.encode_blocks(0, 64) == _orc_encode(2, 0)[::-1]).all()
    c5i, exp = _ds_case(0)
    assert (seam.determine_selectors(np.ascontiguousarray(c5i[::-1]), 0) == exp[::-1]).all()
    info, clusters, exp, _ = _refine_case("shared", 1)
    assert (seam.refine(np.ascontiguousarray(info[::-1]), clusters, 1) == exp[::-1]).all()


# ----------------------------------------------------------------------------- the error convention

def test_error_convention(seam, tiles, request):
    """Failures return 0, leave a text in bu_hip_last_error and the outputs untouched; nothing throws or aborts (basisu_opencl.h, opencl.cpp:972-976); the next valid
    call on the same context succeeds and is right. Every refusal here is decided on the host, before anything is copied or launched."""
    n = 95
    request.addfinalizer(seam.restore)
    c5i, ds_exp = _ds_case(1)
    r_info, r_clusters, r_exp, _ = _refine_case("plain", 1)
    f_info, f_sel, f_idx, f_exp, _ = _fosc_case(1)
    r_info, f_info, c5i = np.ascontiguousarray(r_info[:n]), np.ascontiguousarray(f_info[:n]), np.ascontiguousarray(c5i[:n])
    p_lists = _exact_lists()[:6]
    p_cl, p_px, p_w = _pixel_layout(p_lists)
    p_prm, _ = _orc_fit("exact", 1, 1)

    def all_good():
        assert (seam.encode_blocks(1, 16) == _orc_encode(1, 1)[:n]).all()
        assert (seam.determine_selectors(c5i, 1) == ds_exp[:n]).all()
        assert (seam.refine(r_info, r_clusters, 1) == r_exp[:n]).all()
        assert (seam.fosc(f_info, f_sel, f_idx, 1) == f_exp[:n]).all()
        got = seam.pixel_clusters(p_cl, p_px, p_w, 1, 16)
        assert (got[:, :3] >> 3 == p_prm[:6, :3]).all() and (got[:, 3] >> 5 == p_prm[:6, 3]).all()

    # no pixel blocks set: the four that read tiles refuse (the output size is still what n tiles would need); pixel clusters bring their own pixels and work
    seam.n = n
    assert seam.lib.set_pixel_blocks_device(seam.h, 0, None) == 1
    assert "no pixel blocks" in seam.encode_blocks(1, 16, expect_ok=False)
    assert "no pixel blocks" in seam.determine_selectors(c5i, 1, expect_ok=False)
    assert "no pixel blocks" in seam.refine(r_info, r_clusters, 1, expect_ok=False)
    assert "no pixel blocks" in seam.fosc(f_info, f_sel, f_idx, 1, expect_ok=False)
    seam.pixel_clusters(p_cl, p_px, p_w, 1, 16)
    for fn, args in ((seam.lib.encode_etc1s_blocks, (None, 1, 16)), (seam.lib.determine_selectors, (None, None, 1)),
                     (seam.lib.refine_endpoint_clusterization, (None, 0, None, None, None, 1)),
                     (seam.lib.find_optimal_selector_clusters_for_each_block, (None, 0, None, None, None, 1)),
                     (seam.lib.encode_etc1s_pixel_clusters, (None, 1, None, 0, None, None, 1, 16))):
        assert fn(None, *args) == 0      # no context: 0, nothing to leave a text in
    seam.adopt(seam.d_all, n)
    all_good()

    def refused(call, *words):
        err = call()
        assert all(w in err for w in words), err
        all_good()      # the next valid calls on the same context

    # refine: a window past the end; a current cluster that is not in its window; an empty window; null pointers with counts (the window limit: test_refine_window_limit)
    bad = r_info.copy(); bad[40]["num_clusters"] = r_clusters.size + 1
    refused(lambda: seam.refine(bad, r_clusters, 1, expect_ok=False), "refine", "past the end")
    bad = r_info.copy(); bad[3]["first_cluster_ofs"] = 65535; bad[3]["num_clusters"] = 65535
    refused(lambda: seam.refine(bad, r_clusters, 1, expect_ok=False), "refine", "past the end")
    foreign = int(r_clusters["cluster_index"][(int(r_info[7]["first_cluster_ofs"]) + int(r_info[7]["num_clusters"])) % r_clusters.size])
    bad = r_info.copy(); bad[7]["cur_cluster_index"] = foreign
    refused(lambda: seam.refine(bad, r_clusters, 1, expect_ok=False), "refine", "current cluster")
    bad = r_info.copy(); bad[94]["num_clusters"] = 0
    refused(lambda: seam.refine(bad, r_clusters, 1, expect_ok=False), "refine", "empty")
    refused(lambda: seam.refine(None, r_clusters, 1, expect_ok=False), "refine", "null")
    refused(lambda: seam.lib.refine_endpoint_clusterization(seam.h, vp(r_info), r_clusters.size, None, None, None, 1) == 0 and seam.lib.last_error(seam.h), "null")
    # fosc
    bad = f_info.copy(); bad[0]["num_selectors"] = f_sel.size + 1
    refused(lambda: seam.fosc(bad, f_sel, f_idx, 1, expect_ok=False), "fosc", "past the end")
    bad = f_info.copy(); bad[50]["first_selector"] = 0xFFFFFFFF
    refused(lambda: seam.fosc(bad, f_sel, f_idx, 1, expect_ok=False), "fosc", "past the end")
    bad = f_info.copy(); bad[94]["num_selectors"] = 0
    refused(lambda: seam.fosc(bad, f_sel, f_idx, 1, expect_ok=False), "fosc", "empty")
    refused(lambda: seam.fosc(f_info, f_sel, None, 1, expect_ok=False), "fosc", "null")
    refused(lambda: seam.lib.find_optimal_selector_clusters_for_each_block(seam.h, vp(f_info), f_sel.size, None, vp(f_idx), None, 1) == 0 and seam.lib.last_error(seam.h), "null")
    # pixel clusters
    bad = p_cl.copy(); bad[5]["total_pixels"] += 1
    refused(lambda: seam.pixel_clusters(bad, p_px, p_w, 1, 16, expect_ok=False), "out of range")
    refused(lambda: seam.pixel_clusters(p_cl, p_px, p_w, 1, 16, total_pixels=p_px.shape[0] - 1, expect_ok=False), "out of range")
    zero = p_w.copy(); f, c = int(p_cl[2]["first_pixel_index"]), int(p_cl[2]["total_pixels"]); zero[f:f + c] = 0
    refused(lambda: seam.pixel_clusters(p_cl, p_px, zero, 1, 16, expect_ok=False), "empty")
    huge = p_w.copy(); huge[0] = 2 ** 31
    refused(lambda: seam.pixel_clusters(p_cl, p_px, huge, 1, 16, expect_ok=False), "too large")
    huge = p_w.copy()
    for i in range(3):      # each cluster within the bound (2^30 texels, one repeat), the call over it
        f, c = int(p_cl[i]["first_pixel_index"]), int(p_cl[i]["total_pixels"])
        huge[f:f + c] = 0; huge[f] = 2 ** 30
    refused(lambda: seam.pixel_clusters(p_cl, p_px, huge, 1, 16, expect_ok=False), "texels after expansion")
    refused(lambda: seam.pixel_clusters(p_cl, p_px, None, 1, 16, expect_ok=False), "null")
    refused(lambda: seam.lib.encode_etc1s_pixel_clusters(seam.h, None, p_cl.size, vp(p_cl), p_px.shape[0], vp(p_px), vp(p_w), 1, 16) == 0 and seam.lib.last_error(seam.h), "null")


def test_refine_window_limit(seam, tiles, request):
    """255 distinct windows are served, the 256th is refused on the host -- and 300 blocks that alternate between two windows with ONE first offset are two windows"""
    request.addfinalizer(seam.restore)
    n, k = 300, 300
    info, clusters, exp, block_cluster = _refine_case("plain", 1)    # clusters: 300 flat entries, cluster index = position
    t = tiles
    params = np.stack([clusters["unscaled_color"]["r"], clusters["unscaled_color"]["g"], clusters["unscaled_color"]["b"], clusters["etc_inten"]], axis=1).astype(np.uint8)
    params = np.ascontiguousarray(params)

    def run(wins_of_block, cur):
        w = np.asarray(wins_of_block, np.int64)
        inf = np.zeros(n, BU_BLOCK_INFO)
        inf["first_cluster_ofs"], inf["num_clusters"], inf["cur_cluster_index"], inf["cur_cluster_etc_inten"] = w[:, 0], w[:, 1], cur, params[cur, 3]
        uniq, inv = np.unique(w, axis=0, return_inverse=True)
        return inf, uniq, inv.reshape(-1)

    def expected(uniq, inv, cur):
        coffs, cidx = csr_from_lists([np.arange(f, f + c, dtype=np.uint32) for f, c in uniq])
        e = np.zeros(n, np.uint32)
        oracle().orc_refine_endpoint_clusterization(ptr(t), n, ptr(cur.astype(np.uint32), u32p), ptr(params), k, len(uniq), ptr(coffs, u32p), ptr(cidx, u32p),
                                                    ptr(inv.astype(np.uint8)), 1, ptr(e, u32p))
        return e

    seam.adopt(seam.d_all, n)
    # alternating (0, 150) / (0, 300): the current cluster sits in the shared part
    cur = np.arange(n) % 150
    inf, uniq, inv = run([(0, 150) if b & 1 else (0, 300) for b in range(n)], cur)
    assert len(uniq) == 2
    assert (seam.refine(inf, clusters, 1) == expected(uniq, inv, cur)).all()
    # 255 windows (b, 30 + b % 5) for the first 255 blocks, reused by the rest
    wins = [(b % 255, 30 + (b % 255) % 5) for b in range(n)]
    cur = np.array([f + (b * 7) % c for b, (f, c) in enumerate(wins)])
    inf, uniq, inv = run(wins, cur)
    assert len(uniq) == 255
    assert (seam.refine(inf, clusters, 1) == expected(uniq, inv, cur)).all()
    wins[299] = (255, 30)
    cur[299] = 260
    inf, uniq, inv = run(wins, cur)
    assert len(uniq) == 256
    assert "255" in seam.refine(inf, clusters, 1, expect_ok=False)
