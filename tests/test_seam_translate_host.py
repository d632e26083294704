"""Property tests of csrc/host/seam_translate.h: the host translations between the layouts of section 1 of include/basisu_hip.h (= the reference's
encoder/basisu_opencl.h) and the device-resident layer's tables. No GPU and no oracle: each property is stated over the INPUT, which the test builds itself.

The refusals at the end are the texts bu_hip_last_error reports when the real entry points get the same input (tests/test_gpu_seam_section1.py)."""
import math

import numpy as np
import pytest

from helpers import (BU_BLOCK_INFO, BU_ENDPOINT_CLUSTER, BU_FOSC_BLOCK, BU_FOSC_SELECTOR, BU_PIXEL_CLUSTER, BU_COLOR, ptr, seam_translate_host,
                     seam_refine_tables, seam_fosc_tables, seam_pixel_tables)


# ----------------------------------------------------------------------------- refine

def _flat_clusters(entries, rng):
    """entries: the m_cluster_index of every flat position -> BU_ENDPOINT_CLUSTER array with colours / tables that differ from position to position"""
    cl = np.zeros(len(entries), BU_ENDPOINT_CLUSTER)
    cl["cluster_index"] = entries
    for ch in "rgb":
        cl["unscaled_color"][ch] = rng.integers(0, 32, len(entries))
    cl["etc_inten"] = rng.integers(0, 8, len(entries))
    return cl


def _refine_info(block_windows, clusters, rng, cur=None):
    """block_windows: (first, count) per block; the current cluster is a random member of the window unless given"""
    info = np.zeros(len(block_windows), BU_BLOCK_INFO)
    for b, (f, c) in enumerate(block_windows):
        info[b]["first_cluster_ofs"], info[b]["num_clusters"] = f, c
        info[b]["cur_cluster_index"] = clusters["cluster_index"][f + rng.integers(0, c)] if cur is None else cur[b]
    return info


def _check_refine(info, clusters, tables, n_parents=None):
    offs, idx, bp, cur, params = (tables[k] for k in ("cand_offsets", "cand_indices", "block_parent", "block_cur", "params"))
    assert offs[0] == 0 and offs[-1] == idx.size and bp.size == info.size == cur.size and params.size == clusters.size
    if n_parents is not None:
        assert offs.size - 1 == n_parents
    for b in range(info.size):
        f, c = int(info[b]["first_cluster_ofs"]), int(info[b]["num_clusters"])
        p = int(bp[b])
        assert p < offs.size - 1
        pos = idx[offs[p]:offs[p + 1]]
        want = clusters[f:f + c]
        # the parent's list, mapped back through the flat array, is the window's (cluster index, r, g, b, inten) sequence in order
        got = clusters[pos]
        assert pos.size == c and (got == want).all()
        prm = params[pos]
        assert (prm & 255 == want["unscaled_color"]["r"]).all() and ((prm >> 8) & 255 == want["unscaled_color"]["g"]).all()
        assert ((prm >> 16) & 255 == want["unscaled_color"]["b"]).all() and (prm >> 24 == want["etc_inten"]).all()
        # the current position is an entry of the window and names the current cluster
        assert f <= cur[b] < f + c and clusters[cur[b]]["cluster_index"] == info[b]["cur_cluster_index"]


def _reference_layout(rng, sizes):
    """parents laid end to end, ascending cluster index inside each (frontend.cpp:971-996, 1684-1750) -> (flat entries, (first, count) per parent)"""
    ids = rng.permutation(sum(sizes))
    entries, wins, at = [], [], 0
    for s in sizes:
        entries += sorted(ids[at:at + s].tolist())
        wins.append((at, s))
        at += s
    return entries, wins


def test_refine_reference_layout():
    rng = np.random.default_rng(1)
    entries, wins = _reference_layout(rng, [40, 1, 17, 90, 33, 64, 55])
    cl = _flat_clusters(entries, rng)
    info = _refine_info([wins[i] for i in rng.integers(0, len(wins), 500)], cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=len(wins))


def test_refine_empty_parent_between_two_others():
    """parents A (0, 5), B (5, 0), C (5, 7): B holds no cluster, hence no block; A, C and the window (5, 3) nested in C share offsets without evicting each other"""
    rng = np.random.default_rng(2)
    cl = _flat_clusters(list(range(12)), rng)
    wins = [(0, 5), (5, 7), (5, 3), (0, 5), (5, 3), (5, 7)] * 20
    info = _refine_info(wins, cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=3)
    # a block filed under the empty parent has no current cluster to stand on: refused
    bad = info.copy(); bad[7]["first_cluster_ofs"], bad[7]["num_clusters"] = 5, 0
    t, err = seam_refine_tables(bad, cl)
    assert t is None and "empty" in err


def test_refine_nested_windows():
    rng = np.random.default_rng(3)
    cl = _flat_clusters(list(range(10)), rng)
    info = _refine_info([(0, 5), (0, 10), (0, 10), (0, 5), (0, 10)] * 9, cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=2)


def test_refine_cluster_in_three_windows():
    """cluster 7 at positions 2, 5 and 11 of three windows: every block's current position is the one inside ITS window"""
    rng = np.random.default_rng(4)
    entries = [1, 3, 7, 9,   2, 7, 8,   0, 4, 5, 6, 7, 10]
    cl = _flat_clusters(entries, rng)
    wins = [(0, 4), (4, 3), (7, 6)]
    bw = [wins[i % 3] for i in range(60)]
    info = _refine_info(bw, cl, rng, cur=[7 if i % 2 else entries[wins[i % 3][0]] for i in range(60)])
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=3)
    assert set(t["block_cur"][1::2].tolist()) == {2, 5, 11}


def test_refine_alternating_windows_with_one_first_offset():
    """300 blocks alternating between (0, 5) and (0, 10): two parents. (A map keyed by the first offset alone makes a "new" window at every switch and
    refuses the call with "more than 255 distinct candidate windows".)"""
    rng = np.random.default_rng(5)
    cl = _flat_clusters(list(range(10)), rng)
    info = _refine_info([(0, 5) if b & 1 else (0, 10) for b in range(300)], cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None, err
    _check_refine(info, cl, t, n_parents=2)


def test_refine_255_windows_and_256():
    rng = np.random.default_rng(6)
    cl = _flat_clusters(list(range(300)), rng)
    assert seam_translate_host().st_max_windows() == 255
    wins = [(i, 1 + i % 7) for i in range(256)]
    info = _refine_info(wins[:255] * 2, cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=255)
    info = _refine_info(wins + wins[:10], cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert t is None and "255" in err


def test_refine_flat_list_beyond_65535_entries():
    """the last window starts at 65,000 and is 2,000 long: offsets and counts are 16-bit, the flat positions are not"""
    rng = np.random.default_rng(7)
    entries = (np.arange(67000) % 65536).astype(np.uint16)     # 65,000 .. 66,999 hold 65,000 .. 65,535, 0 .. 1,463: distinct inside the window
    cl = _flat_clusters(entries, rng)
    info = _refine_info([(65000, 2000), (0, 300), (65000, 2000), (64000, 1000)] * 25, cl, rng)
    t, err = seam_refine_tables(info, cl)
    assert err is None
    _check_refine(info, cl, t, n_parents=3)
    assert t["block_cur"].max() > 65535


# ----------------------------------------------------------------------------- fosc

def _unpack_selectors(block8):
    """the selector unpacking of oracle/etc1s_oracle.c unpack_etc1s (etc.h:232-236): -> sel[p], p = y * 4 + x"""
    v = int.from_bytes(bytes(block8), "big")
    to_sel = [2, 3, 1, 0]
    sel = []
    for p in range(16):
        x, y = p & 3, p >> 2
        bit = x * 4 + y
        sel.append(to_sel[((v >> bit) & 1) | (((v >> (16 + bit)) & 1) << 1)])
    return sel


def _selector_words():
    words = [0, 0xFFFFFFFF]
    for p in range(16):
        for s in range(4):
            words.append(s << (2 * p))                               # one position set, the others 0
            words.append((0xFFFFFFFF ^ (3 << (2 * p))) | (s << (2 * p)))   # ... the others 3
    words += np.random.default_rng(8).integers(0, 2 ** 32, 1000, dtype=np.uint64).tolist()
    return np.array(words, np.uint32)


def test_selector_words_round_trip():
    L = seam_translate_host()
    out = np.zeros(8, np.uint8)
    for w in _selector_words().tolist():
        L.st_selectors_to_etc_block(w, ptr(out))
        assert (out[:4] == 0).all()
        assert _unpack_selectors(out) == [(w >> (2 * p)) & 3 for p in range(16)], hex(w)


def test_fosc_windows_and_blocks():
    rng = np.random.default_rng(9)
    sel = np.zeros(1064, BU_FOSC_SELECTOR)
    sel["packed_selectors"] = _selector_words()[:1064]
    wins = [(0, 5), (0, 10), (10, 200), (5, 1), (210, 854), (100, 300)]    # nested, overlapping, shared first offset
    info = np.zeros(400, BU_FOSC_BLOCK)
    for b in range(400):
        info[b]["first_selector"], info[b]["num_selectors"] = wins[(b * 7 + b // 3) % len(wins)]
    for ch in "rgb":
        info["etc_color5_inten"][ch] = rng.integers(0, 32, 400)
    info["etc_color5_inten"]["a"] = rng.integers(0, 8, 400)
    t, err = seam_fosc_tables(info, sel)
    assert err is None
    offs, idx, bp = t["cand_offsets"], t["cand_indices"], t["block_parent"]
    assert offs.size - 1 == len(wins) and offs[-1] == idx.size
    for b in range(400):
        f, c = int(info[b]["first_selector"]), int(info[b]["num_selectors"])
        assert (idx[offs[bp[b]]:offs[bp[b] + 1]] == np.arange(f, f + c)).all()
        _check_color_block(t["encoded_blocks"][b], *[int(info[b]["etc_color5_inten"][ch]) for ch in "rgba"])
    for i in range(sel.size):
        w = int(sel[i]["packed_selectors"])
        assert _unpack_selectors(t["selector_blocks"][i]) == [(w >> (2 * p)) & 3 for p in range(16)]


def test_fosc_alternating_windows_and_window_limit():
    sel = np.zeros(600, BU_FOSC_SELECTOR)
    info = np.zeros(300, BU_FOSC_BLOCK)
    info["first_selector"] = 0
    info["num_selectors"] = np.where(np.arange(300) & 1, 5, 10)
    t, err = seam_fosc_tables(info, sel)
    assert err is None and t["cand_offsets"].size == 3
    info = np.zeros(256, BU_FOSC_BLOCK)
    info["first_selector"] = np.arange(256); info["num_selectors"] = 3
    t, err = seam_fosc_tables(info[:255], sel)
    assert err is None and t["cand_offsets"].size == 256
    t, err = seam_fosc_tables(info, sel)
    assert t is None and "255" in err


# ----------------------------------------------------------------------------- colour5 + inten -> etc_block

def _check_color_block(block8, r5, g5, b5, inten):
    """every field the reference reads back from an ETC1S block (etc.h: get_base5_color, get_inten_table(0 / 1), get_diff_bit, get_flip_bit), plus what
    is_etc1s wants besides: zero deltas; selectors zero"""
    b = [int(v) for v in block8]
    assert [b[0] >> 3, b[1] >> 3, b[2] >> 3] == [r5, g5, b5]            # get_base5_color: the top five bits of bytes 0..2
    assert [b[0] & 7, b[1] & 7, b[2] & 7] == [0, 0, 0]                  # delta3 = 0
    assert (b[3] >> 5) & 7 == inten and (b[3] >> 2) & 7 == inten        # get_inten_table(0), (1)
    assert (b[3] >> 1) & 1 == 1 and b[3] & 1 == 1                       # diff bit, flip bit
    assert b[4:] == [0, 0, 0, 0]


def test_color5_inten_to_etc_block():
    L = seam_translate_host()
    out = np.zeros(8, np.uint8)
    rng = np.random.default_rng(10)
    colours = [(0, 0, 0), (31, 31, 31), (31, 0, 0), (0, 31, 0), (0, 0, 31), (1, 2, 4), (16, 8, 24)]
    colours += [tuple(int(v) for v in c) for c in rng.integers(0, 32, (400, 3))]
    colours += [(r, r, r) for r in range(32)] + [(r, 31 - r, (r * 7) & 31) for r in range(32)]
    for r5, g5, b5 in colours:
        for inten in range(8):
            L.st_color5_inten_to_etc_block(r5, g5, b5, inten, ptr(out))
            _check_color_block(out, r5, g5, b5, inten)


# ----------------------------------------------------------------------------- pixel clusters

def _pixel_input(lists):
    """lists: [(colours (m, 4) u8, weights (m,))] laid end to end -> (BU_PIXEL_CLUSTER array, pixels, weights)"""
    cl = np.zeros(len(lists), BU_PIXEL_CLUSTER)
    at = 0
    for i, (c, w) in enumerate(lists):
        cl[i]["first_pixel_index"], cl[i]["total_pixels"] = at, len(w)
        at += len(w)
    px = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint8).reshape(-1, 4) for c, _ in lists]))
    return cl, px, np.ascontiguousarray(np.concatenate([np.asarray(w, np.uint32) for _, w in lists]))


def _check_pixel_tables(lists, t):
    at_tv = 0
    assert t["offsets"][0] == 0 and t["offsets"][-1] == t["indices"].size and t["texels"].size % 16 == 0
    for c, (col, w) in enumerate(lists):
        n = int(np.sum(w))
        reps = 8 // math.gcd(n, 8)
        assert t["reps"][c] == reps and reps in (1, 2, 4, 8) and t["totals"][c] == n
        tv = t["indices"][t["offsets"][c]:t["offsets"][c + 1]]
        assert tv.size * 8 == n * reps and (tv == at_tv + np.arange(tv.size)).all()
        got = t["texels"][at_tv * 8:(at_tv + tv.size) * 8]
        one = np.repeat(np.ascontiguousarray(np.asarray(col, np.uint8).reshape(-1, 4)).view(np.uint32).reshape(-1), np.asarray(w, np.int64))   # list order, w_i times each
        assert (got == np.tile(one, reps)).all()
        at_tv += tv.size
    assert (t["texels"][at_tv * 8:] == 0).all() and t["texels"].size - at_tv * 8 < 16


def test_pixel_clusters_expansion():
    rng = np.random.default_rng(11)
    lists = []
    for residue in range(8):   # every residue of n mod 8, twice: a few colours with small weights, many colours with large ones
        for m, hi in ((3, 5), (40, 300)):
            w = rng.integers(1, hi, m)
            w[0] += (residue - int(w.sum())) % 8
            assert w.sum() % 8 == residue
            lists.append((rng.integers(0, 256, (m, 4)), w))
    lists.append(([[9, 8, 7, 255]], [1]))                                         # one colour, weight 1: eight copies
    lists.append(([[1, 2, 3, 255], [1, 2, 3, 255], [4, 5, 6, 255]], [3, 0, 2]))   # a colour listed twice, a zero weight inside a non-empty cluster
    lists.append(([[200, 100, 50, 255]], [4097]))
    cl, px, w = _pixel_input(lists)
    t, err = seam_pixel_tables(cl, px, w)
    assert err is None
    _check_pixel_tables(lists, t)
    # clusters need not cover the pixel array in order, or at all
    order = rng.permutation(len(lists))[:11]
    t, err = seam_pixel_tables(np.ascontiguousarray(cl[order]), px, w)
    assert err is None
    _check_pixel_tables([lists[i] for i in order], t)


# ----------------------------------------------------------------------------- refusals: the error, and no tables

def _small_refine():
    rng = np.random.default_rng(12)
    cl = _flat_clusters([3, 5, 6, 9, 1, 2, 8, 11, 12, 20], rng)
    return _refine_info([(0, 4), (4, 6), (0, 4), (4, 6)], cl, rng), cl


def _refused(result, *words):
    tables, err = result
    assert tables is None and err and all(w in err for w in words), err


def test_refusals_refine():
    info, cl = _small_refine()
    assert seam_refine_tables(info, cl)[1] is None
    bad = info.copy(); bad[1]["num_clusters"] = 7                                  # 4 + 7 > 10
    _refused(seam_refine_tables(bad, cl), "past the end")
    bad = info.copy(); bad[2]["first_cluster_ofs"] = 65535; bad[2]["num_clusters"] = 65535
    _refused(seam_refine_tables(bad, cl), "past the end")
    bad = info.copy(); bad[0]["cur_cluster_index"] = 1                              # cluster 1 lives in the OTHER window
    _refused(seam_refine_tables(bad, cl), "current cluster")
    bad = info.copy(); bad[3]["cur_cluster_index"] = 4000                           # ... or nowhere
    _refused(seam_refine_tables(bad, cl), "current cluster")
    _refused(seam_refine_tables(info, cl, null=("info",)), "null")
    _refused(seam_refine_tables(info, cl, null=("clusters",)), "null")
    # nothing to do is not an error
    t, err = seam_refine_tables(info[:0], cl[:0])
    assert err is None and t["cand_offsets"].tolist() == [0]


def test_refusals_fosc():
    sel = np.zeros(10, BU_FOSC_SELECTOR)
    info = np.zeros(4, BU_FOSC_BLOCK)
    info["first_selector"] = [0, 4, 0, 4]; info["num_selectors"] = [4, 6, 4, 6]
    assert seam_fosc_tables(info, sel)[1] is None
    bad = info.copy(); bad[3]["num_selectors"] = 7
    _refused(seam_fosc_tables(bad, sel), "past the end")
    bad = info.copy(); bad[0]["first_selector"] = 0xFFFFFFFF; bad[0]["num_selectors"] = 2     # first + count wraps 32 bits
    _refused(seam_fosc_tables(bad, sel), "past the end")
    bad = info.copy(); bad[2]["num_selectors"] = 0
    _refused(seam_fosc_tables(bad, sel), "empty")
    _refused(seam_fosc_tables(info, sel, null=("info",)), "null")
    _refused(seam_fosc_tables(info, sel, null=("selectors",)), "null")


def test_refusals_pixel_clusters():
    lists = [([[1, 2, 3, 255], [4, 5, 6, 255]], [3, 2]), ([[7, 8, 9, 255]], [5])]
    cl, px, w = _pixel_input(lists)
    assert seam_pixel_tables(cl, px, w)[1] is None
    bad = cl.copy(); bad[1]["total_pixels"] = 2                                     # 2 + 2 > 3
    _refused(seam_pixel_tables(bad, px, w), "out of range")
    bad = cl.copy(); bad[0]["first_pixel_index"] = 2 ** 64 - 1                      # first + count wraps 64 bits
    _refused(seam_pixel_tables(bad, px, w), "out of range")
    _refused(seam_pixel_tables(cl, px, np.array([3, 2, 0], np.uint32)), "empty")   # an all-zero-weight cluster
    _refused(seam_pixel_tables(cl[:1], px, np.array([0, 0, 5], np.uint32)), "empty")
    _refused(seam_pixel_tables(cl, px, np.array([3, 2, 2 ** 31], np.uint32)), "too large")            # one cluster over 2^31 - 1 texels
    _refused(seam_pixel_tables(cl, px, np.array([3, 2, 2 ** 28 + 1], np.uint32)), "too large")        # ... only once repeated eight times
    # every cluster within the bound, the call as a whole over it: refused before anything is expanded
    assert seam_translate_host().st_max_expanded_texels() == 2 ** 31 - 1
    many = np.zeros(3, BU_PIXEL_CLUSTER); many["first_pixel_index"] = 2; many["total_pixels"] = 1
    _refused(seam_pixel_tables(many, px, np.array([3, 2, 2 ** 30], np.uint32)), "texels after expansion")
    for name in ("clusters", "pixels", "weights"):
        _refused(seam_pixel_tables(cl, px, w, null=(name,)), "null")
    t, err = seam_pixel_tables(cl[:0], px, w)
    assert err is None and t["offsets"].tolist() == [0] and t["texels"].size == 0
